"""Rank processes for the fp8 GPU tests (one process = one rank; placement, spawning and the barrier
are tests/gpu_workers.py's).  Expected values: tests/fp8_ref.py, computed in-process from the same
seeded inputs -- never from the library.  Every comparison is byte for byte over every element, two
NaNs of the format counting as equal (fp8_ref.mismatches).
"""
import os
import traceback

import numpy as np

from gpu_workers import use_rank_device

GUARD = 256  # bytes past every recv, filled before the call and checked after it
FILL = 0xAB


def _setup(rank, n, port, env):
    os.environ.update(env)
    os.environ["MINI_NCCL_PORT"] = str(port)
    import fp8_ref as F
    import hip_rt
    import mini_nccl as M
    use_rank_device(rank)
    return hip_rt, M, F, M.Comm(n, rank, "127.0.0.1")


# ---------------------------------------------------------------- 1. every operand pair
def exhaustive_fold(out_q):
    """mncclLocalReduce over all 65 536 (local, incoming) pairs, per format and op: once on
    dword-aligned buffers (the vector kernel) and once with all three pointers one byte further (the
    element kernel).  Result: {(fmt, op, offset): (rc, mismatches, [first few (a, b, got, expected)])}."""
    try:
        import fp8_ref as F
        import hip_rt
        import mini_nccl as M
        hip_rt.set_device(0)
        a = np.repeat(np.arange(256, dtype=np.uint8), 256)
        b = np.tile(np.arange(256, dtype=np.uint8), 256)
        count = a.size
        da, db, dc = (hip_rt.DeviceBuffer(count + 16 + GUARD) for _ in range(3))
        res = {}
        for off in (0, 1):
            da.upload(a, off)
            db.upload(b, off)
            for fmt in F.FORMATS:
                for op in F.OPS:
                    dc.fill_byte(FILL)
                    rc = M.local_reduce(dc.ptr + off, da.ptr + off, db.ptr + off, count, F.code(fmt), F.OP_CODE[op], 0)
                    hip_rt.sync()
                    if rc != 0:
                        res[(fmt, op, off)] = (rc, -1, [])
                        continue
                    whole = dc.download(np.uint8, count + 16 + GUARD)
                    got, exp = whole[off:off + count], F.fold(a, b, fmt, op)
                    bad = (got != exp) & ~(F.is_nan(got, fmt) & F.is_nan(exp, fmt))
                    idx = np.flatnonzero(bad)
                    outside = int((whole[:off] != FILL).sum() + (whole[off + count:] != FILL).sum())
                    res[(fmt, op, off)] = (rc, int(idx.size) + outside,
                                           [(int(a[i]), int(b[i]), int(got[i]), int(exp[i])) for i in idx[:8]])
        for x in (da, db, dc):
            x.free()
        out_q.put((0, {"results": res}))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 2. every input x every scalar
def exhaustive_scale(env, port, out_q):
    """nranks == 1: a pre-multiplied sum is out = encode(s * x).  All 256 inputs under each of the
    256 scalars per format, the ops created and destroyed in turn (at most 16 live at once)."""
    try:
        hip_rt, M, F, comm = _setup(0, 1, port, env)
        st = hip_rt.Stream()
        x = np.arange(256, dtype=np.uint8)
        send, recv = hip_rt.DeviceBuffer(256), hip_rt.DeviceBuffer(256 * 256 + GUARD)
        send.upload(x)
        res = {}
        for fmt in F.FORMATS:
            recv.fill_byte(FILL)
            rcs, live = [], []
            for s in range(256):
                op = comm.redop_premul_sum(s, F.code(fmt))  # an int: the 8 bits
                live.append(op)
                rcs.append(comm.all_reduce(send.ptr, recv.ptr + 256 * s, 256, F.code(fmt), op, st.handle))
                if len(live) == 16:
                    rcs += [comm.redop_destroy(h) for h in live]
                    live = []
            st.sync()
            whole = recv.download(np.uint8, 256 * 256 + GUARD)
            got = whole[:65536].reshape(256, 256)
            exp = np.stack([F.scale(x, s, fmt) for s in range(256)])
            bad, first = F.mismatches(got.reshape(-1), exp.reshape(-1), fmt)
            res[fmt] = {"rcs": sorted(set(rcs)), "bad": bad + int((whole[65536:] != FILL).sum()),
                        "first": (first // 256, first % 256, int(got.reshape(-1)[first]), int(exp.reshape(-1)[first])) if bad else None,
                        "algo": comm.info()["last_algo"]}
        send.free()
        recv.free()
        st.destroy()
        out_q.put((0, {"results": res, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 3 / 4. the folding collectives
def expected(F, case, xs, rank, stats=None):
    fmt, op, s = case["fmt"], case["op"], case.get("s")
    if case["coll"] == "ar":
        return F.allreduce_expect(xs, fmt, op, rank, s, stats)
    if case["coll"] == "rs":
        return F.reduce_scatter_expect(xs, fmt, op, rank, s, stats)
    return F.reduce_expect(xs, fmt, op, s, stats)


def case_count(case, n):
    """Elements of the send buffer: n chunks (and the all-reduce's tail)."""
    return n * case["chunk"] + (case.get("tail", 0) if case["coll"] == "ar" else 0)


def fold_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator.  A case: coll ("ar" / "rs" / "rd"), fmt, op (one of the four,
    or "premul" with the scalar's code s), chunk (elements per chunk), tail (all-reduce only),
    inplace, algo, root, seed, kind (fp8_ref.inputs), mem (device / pinned / pageable)."""
    try:
        hip_rt, M, F, comm = _setup(rank, n, port, env)
        stream = hip_rt.Stream()
        results = []
        for case in cases:
            coll, fmt, c = case["coll"], case["fmt"], case["chunk"]
            inplace, root = case.get("inplace", False), case.get("root", 0)
            comm.set_algo(case["algo"])
            dt = F.code(fmt)
            ns = case_count(case, n)
            nr = c if coll == "rs" else ns
            mine = rank * c if coll == "rs" else 0
            mem = case.get("mem", "device")
            if inplace:
                whole = hip_rt.buffer(mem, ns + GUARD)
                send, recv = hip_rt.View(whole, 0, ns), hip_rt.View(whole, mine, nr)
                guard = hip_rt.View(whole, ns, GUARD)
            else:
                sbuf, rbuf = hip_rt.buffer(mem, ns), hip_rt.buffer(mem, nr + GUARD)
                send, recv = hip_rt.View(sbuf, 0, ns), hip_rt.View(rbuf, 0, nr)
                guard = hip_rt.View(rbuf, nr, GUARD)
                rbuf.fill_byte(FILL)
            xs = F.inputs(n, ns, fmt, case["seed"], case["kind"])
            exp = expected(F, case, xs, rank)
            send.upload(xs[rank])
            guard.upload(np.full(GUARD, FILL, np.uint8))
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            g0 = comm.info()["read_grid_calls"]
            premul = case["op"] == "premul"
            op = comm.redop_premul_sum(int(case["s"]), dt) if premul else F.OP_CODE[case["op"]]
            if coll == "rs":
                rc = comm.reduce_scatter(send.ptr, recv.ptr, c, dt, op, stream.handle)
            elif coll == "rd":
                rc = comm.reduce(send.ptr, recv.ptr, ns, dt, op, root, stream.handle)
            else:
                rc = comm.all_reduce(send.ptr, recv.ptr, ns, dt, op, stream.handle)
            drc = comm.redop_destroy(op) if premul else 0
            stream.sync()
            ci = comm.info()
            bad, first, detail = -1, -1, ""
            if rc == 0:
                bad = 0
                if coll != "rd" or rank == root:
                    got = recv.download(np.uint8, nr)
                    bad, first = F.mismatches(got, exp, fmt)
                    if bad:
                        detail = f"got {got[first]:#x} expected {exp[first]:#x}"
                elif not inplace:  # a non-root's recv is never touched
                    bad = int((recv.download(np.uint8, nr) != FILL).sum())
                bad += int((guard.download(np.uint8, GUARD) != FILL).sum())
            results.append({"case": case, "rc": rc, "destroy_rc": drc, "bad": bad, "first": first, "detail": detail,
                            "algo": ci["last_algo"], "grid": ci["read_grid_calls"] - g0, "async": comm.async_error()})
            if inplace:
                whole.free()
            else:
                sbuf.free()
                rbuf.free()
        stream.destroy()
        out_q.put((rank, {"results": results, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def window_rank(rank, n, port, env, out_q, barrier=None):
    """One all-reduce inside registered windows, launched without a rendezvous."""
    try:
        hip_rt, M, F, comm = _setup(rank, n, port, env)
        st = hip_rt.Stream()
        wbytes = 1 << 20
        sbuf, rbuf = hip_rt.DeviceBuffer(wbytes, fresh=True), hip_rt.DeviceBuffer(wbytes, fresh=True)
        comm.register(sbuf.ptr, wbytes)
        comm.register(rbuf.ptr, wbytes)
        fmt, count, so, ro = "e4m3", 3 * 20004 + 2, 256, 4096
        xs = F.inputs(n, count, fmt, 9100, "wild")
        rbuf.fill_byte(FILL)
        sbuf.upload(xs[rank], so)
        hip_rt.sync()
        barrier.wait(120)
        w0 = comm.info()["window_calls"]
        rc = comm.all_reduce(sbuf.ptr + so, rbuf.ptr + ro, count, F.code(fmt), M.ncclSum, st.handle)
        st.sync()
        whole = rbuf.download(np.uint8, wbytes)
        bad = F.mismatches(whole[ro:ro + count], F.allreduce_expect(xs, fmt, "sum", rank), fmt)[0]
        bad += int((whole[:ro] != FILL).sum() + (whole[ro + count:] != FILL).sum())
        ci = comm.info()
        res = {"rc": rc, "bad": bad, "wc": ci["window_calls"] - w0, "algo": ci["last_algo"], "fast": ci["window_fast"]}
        st.destroy()
        res["destroy"] = comm.destroy()
        sbuf.free()
        rbuf.free()
        out_q.put((rank, res))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def graph_rank(rank, n, port, env, replays, out_q):
    """One all-reduce captured into a HIP graph on the read schedule, replayed on fresh inputs."""
    try:
        hip_rt, M, F, comm = _setup(rank, n, port, env)
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        fmt, count = "e5m2", (1 << 16) + 3
        send, recv = hip_rt.DeviceBuffer(count), hip_rt.DeviceBuffer(count)
        rcs = []
        g = hip_rt.Graph(st, lambda: rcs.append(comm.all_reduce(send.ptr, recv.ptr, count, F.code(fmt), M.ncclSum, st.handle)))
        captured_algo = comm.info()["last_algo"]
        bad = []
        for k in range(replays):
            xs = F.inputs(n, count, fmt, 9200 + k, "wild")
            send.upload(xs[rank])
            hip_rt.sync()
            g.launch()
            st.sync()
            bad.append(F.mismatches(recv.download(np.uint8, count), F.allreduce_expect(xs, fmt, "sum", rank), fmt)[0])
        g.destroy()
        out_q.put((rank, {"capture_rc": rcs, "bad": bad, "captured_algo": captured_algo, "async": comm.async_error()}))
        send.free()
        recv.free()
        st.destroy()
        comm.destroy()
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


# ---------------------------------------------------------------- 5. the calls that only move bytes
def payload(seed, rank, nbytes):
    """Rank `rank`'s send bytes of a case: uniform over all 256 codes, computed alike on every rank."""
    return np.random.default_rng([seed, rank]).integers(0, 256, nbytes, dtype=np.uint8)


def v_matrix(n, count):
    """ncclAllToAllv's matrix at n ranks: counts[r][q] elements from r to q -- a zero block, a 1-byte
    block, the rest around `count` -- and odd displacements: block q of a send starts one byte past
    an odd boundary, the blocks of a recv are packed with 3-byte gaps."""
    counts = [[count - 7 * ((r + 2 * q) % 3) for q in range(n)] for r in range(n)]
    counts[0][1] = 0
    counts[1][2 % n] = 1
    sdispls = [[q * (count + 5) + 1 for q in range(n)] for r in range(n)]
    rdispls = []
    for q in range(n):  # receiver q: the block from r
        at, row = 3, []
        for r in range(n):
            row.append(at)
            at += counts[r][q] + 3
        rdispls.append(row)
    return counts, sdispls, rdispls


def mover_rank(rank, n, port, cases, env, out_q, barrier=None):
    """The calls that do no arithmetic, with an fp8 datatype.  A case: coll ("ag", "bc", "a2a", "ga",
    "sc", "a2av"), fmt, count, algo, root, seed.  Every recv is compared whole: the blocks hold the
    senders' bytes, everything else (and the guard) its fill."""
    try:
        hip_rt, M, F, comm = _setup(rank, n, port, env)
        st = hip_rt.Stream()
        results = []
        for case in cases:
            coll, count, root, seed = case["coll"], case["count"], case.get("root", 0), case["seed"]
            dt = F.code(case["fmt"])
            comm.set_algo(case["algo"])
            big = n * count
            if coll == "a2av":
                counts, sd, rd = v_matrix(n, count)
                sbytes = max(sd[rank][q] + counts[rank][q] for q in range(n)) + 8
                rbytes = rd[rank][n - 1] + counts[n - 1][rank] + 8
            else:
                sbytes = {"ag": count, "bc": count, "a2a": big, "ga": count, "sc": big}[coll]
                rbytes = {"ag": big, "bc": count, "a2a": big, "ga": big, "sc": count}[coll]
            sbuf, rbuf = hip_rt.DeviceBuffer(sbytes), hip_rt.DeviceBuffer(rbytes + GUARD)
            xs = [payload(seed, q, sbytes) for q in range(n)]  # (every rank's send has this rank's size or is unused)
            want = np.full(rbytes + GUARD, FILL, np.uint8)
            if coll == "ag":
                want[:big] = np.concatenate([payload(seed, q, count) for q in range(n)])
            elif coll == "bc":
                want[:count] = payload(seed, root, count)
            elif coll == "a2a":
                for q in range(n):
                    want[q * count:(q + 1) * count] = payload(seed, q, big)[rank * count:(rank + 1) * count]
            elif coll == "ga":
                if rank == root:
                    want[:big] = np.concatenate([payload(seed, q, count) for q in range(n)])
            elif coll == "sc":
                want[:count] = payload(seed, root, big)[rank * count:(rank + 1) * count]
            else:
                for r in range(n):
                    sb = max(sd[r][q] + counts[r][q] for q in range(n)) + 8
                    src = payload(seed, r, sb)
                    want[rd[rank][r]:rd[rank][r] + counts[r][rank]] = src[sd[r][rank]:sd[r][rank] + counts[r][rank]]
            sbuf.upload(xs[rank])
            rbuf.fill_byte(FILL)
            hip_rt.sync()
            barrier.wait(120)
            if coll == "ag":
                rc = comm.all_gather(sbuf.ptr, rbuf.ptr, count, dt, st.handle)
            elif coll == "bc":
                rc = comm.broadcast(sbuf.ptr if rank == root else None, rbuf.ptr, count, dt, root, st.handle)
            elif coll == "a2a":
                rc = comm.all_to_all(sbuf.ptr, rbuf.ptr, count, dt, st.handle)
            elif coll == "ga":
                rc = comm.gather(sbuf.ptr, rbuf.ptr if rank == root else None, count, dt, root, st.handle)
            elif coll == "sc":
                rc = comm.scatter(sbuf.ptr if rank == root else None, rbuf.ptr, count, dt, root, st.handle)
            else:
                rc = comm.all_to_all_v(sbuf.ptr, counts[rank], sd[rank], rbuf.ptr, [counts[r][rank] for r in range(n)],
                                       rd[rank], dt, st.handle)
            st.sync()
            got = rbuf.download(np.uint8, rbytes + GUARD)
            results.append({"case": case, "rc": rc, "bad": int((got != want).sum()), "algo": comm.info()["last_algo"],
                            "async": comm.async_error()})
            sbuf.free()
            rbuf.free()
        st.destroy()
        out_q.put((rank, {"results": results, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def p2p_ring_rank(rank, n, port, counts, env, out_q, barrier=None):
    """A grouped ncclSend to rank + 1 / ncclRecv from rank - 1 per count, once into a registered
    window (the sender pushes direct) and once into a buffer outside it (through the scratch)."""
    try:
        hip_rt, M, F, comm = _setup(rank, n, port, env)
        st = hip_rt.Stream()
        wb = 1 << 16
        win, plain, send = (hip_rt.DeviceBuffer(wb, fresh=True) for _ in range(3))
        comm.register(win.ptr, wb)
        nxt, prv = (rank + 1) % n, (rank - 1) % n
        results = []
        for i, count in enumerate(counts):
            for where, buf in (("win", win), ("plain", plain)):
                off = 64 + 16 * i
                want = np.full(wb, FILL, np.uint8)
                want[off:off + count] = payload(9300 + i, prv, count)
                send.upload(payload(9300 + i, rank, count))
                buf.fill_byte(FILL)
                hip_rt.sync()
                barrier.wait(120)
                d0 = comm.info()["p2p_direct_recvs"]
                dt = F.code(("e4m3", "e5m2")[i % 2])
                with M.group() as g:
                    rcs = [comm.send(send.ptr, count, dt, nxt, st.handle), comm.recv(buf.ptr + off, count, dt, prv, st.handle)]
                st.sync()
                results.append({"count": count, "where": where, "rcs": rcs + [g.rc],
                                "bad": int((buf.download(np.uint8, wb) != want).sum()),
                                "direct": comm.info()["p2p_direct_recvs"] - d0, "async": comm.async_error()})
        st.destroy()
        rc = comm.destroy()
        for b in (win, plain, send):
            b.free()
        out_q.put((rank, {"results": results, "destroy": rc}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
