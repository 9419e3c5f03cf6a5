"""Rank processes for the ncclBroadcast / ncclReduce GPU tests (one process = one rank; placement,
spawning and comparison are tests/gpu_workers.py's, the three unrooted collectives' buffers and
expectations tests/coll_workers.py's).

Expected values, computed in-process from the same seeded inputs: a Broadcast's every rank holds
the root's input; a Reduce's root holds rooted_ref.reduce_expect (per chunk of ceil(count / n)
elements the oracle's fold in the all-reduce's order); nobody else's recv is touched.
"""
import ctypes
import os
import time
import traceback

import numpy as np

import coll_workers as CW
from coll_workers import GUARD, _info_fields
from gpu_workers import compare, make_inputs, testkern, use_rank_device

FILL = 0xAB  # guard bytes and the buffers a rank's role does not use


def rank_inputs(n, count, dtype, seed, special, ranks):
    """make_inputs' buffers of the given ranks only (rank r's is seeded seed + r)."""
    import oracle_api as O
    if special:
        xs = make_inputs(n, count, dtype, seed, True)
        return {r: xs[r] for r in ranks}
    return {r: O.random_inputs(1, count, dtype, seed=seed + r)[0] for r in ranks}


def _placement(case, key, dflt, rank):
    m = case.get(key, dflt)
    return m[rank % len(m)] if isinstance(m, (list, tuple)) else m


def _rooted_case(comm, case, rank, n, stream, barrier, rng):
    """One Broadcast ("bc") / Reduce ("rd") case: count elements, root, inplace (on the root),
    null (a non-root passes NULL for the buffer its role does not use; otherwise a FILL-filled
    buffer, which must come back unchanged), offset / recv_offset (each a value or a per-rank list;
    recv_offset defaults to offset), special, calls, mem / recv_mem, skew_ms."""
    import hip_rt
    import oracle_api as O
    import rooted_ref
    coll, dtype, op, c, root = case["coll"], case["dtype"], case.get("op", "sum"), case["count"], case["root"]
    inplace, seed, (off, roff) = case.get("inplace", False), case.get("seed", 1), CW.offsets(case, rank)
    code, npd = O.DTYPES[dtype]
    nb = c * np.dtype(npd).itemsize
    is_root = rank == root
    uses_send = coll == "rd" or is_root
    uses_recv = coll == "bc" or is_root
    mem_s = _placement(case, "mem", "device", rank)
    mem_r = _placement(case, "recv_mem", mem_s, rank)
    bufs = []
    if is_root and inplace:
        whole = hip_rt.buffer(mem_s, nb + off + GUARD)
        bufs.append(whole)
        send = recv = hip_rt.View(whole, off, nb)
        guard = hip_rt.View(whole, off + nb, GUARD)
        spare = None
    else:
        # the unused side: NULL, or a FILL-filled buffer (with its guard) that nobody may write
        sbuf = hip_rt.buffer(mem_s, nb + off + GUARD) if uses_send or not case.get("null") else None
        rbuf = hip_rt.buffer(mem_r, nb + roff + GUARD) if uses_recv or not case.get("null") else None
        bufs += [b for b in (sbuf, rbuf) if b is not None]
        for b in bufs:
            b.fill_byte(FILL)
        send = hip_rt.View(sbuf, off, nb) if sbuf is not None else None
        recv = hip_rt.View(rbuf, roff, nb) if rbuf is not None else None
        guard = hip_rt.View(rbuf, roff + nb, GUARD) if uses_recv else None
        spare = None if (uses_send and uses_recv) else (rbuf if uses_send else sbuf)
    bad, first, detail, rc, algos = 0, -1, "", 0, []
    t0 = time.time()
    for k in range(case.get("calls", 1)):
        need = set(range(n)) if (coll == "rd" and is_root) else {root} | ({rank} if uses_send else set())
        xs = rank_inputs(n, c, dtype, seed + 1000 * k, case.get("special", False), need)
        if uses_send:
            send.upload(xs[rank])
        if guard is not None:
            guard.upload(np.full(GUARD, FILL, np.uint8))
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        if case.get("skew_ms"):
            time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
        sp = send.ptr if send is not None else None
        rp = recv.ptr if recv is not None else None
        if coll == "bc":
            rc = comm.broadcast(sp, rp, c, code, root, stream.handle)
        else:
            rc = comm.reduce(sp, rp, c, code, O.OPS[op], root, stream.handle)
        if rc != 0:
            bad = -1
            break
        stream.sync()
        algos.append(comm.info()["last_algo"])
        b = 0
        if uses_recv:
            exp = xs[root] if coll == "bc" else rooted_ref.reduce_expect([xs[q] for q in range(n)], dtype, op)
            got = recv.download(npd, c)
            b, f = compare(got, exp, dtype, coll == "rd" and op in ("sum", "prod"))
            if b and not bad:
                first, detail = f, f"call {k}: got {got[f]!r} expected {exp[f]!r}"
            b += int((guard.download(np.uint8, GUARD) != FILL).sum())  # nothing written past recv
        if coll == "rd" and not (is_root and inplace):
            # a Reduce never writes a send buffer
            b += compare(send.download(npd, c), xs[rank], dtype, False)[0]
        if spare is not None:  # the unused buffer, whole: unchanged
            b += int((spare.download(np.uint8, spare.nbytes) != FILL).sum())
        bad += b
    res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos, "secs": time.time() - t0}
    res.update(_info_fields(comm))
    for b in bufs:
        b.free()
    return res


def _unrooted_case(comm, case, rank, n, stream, barrier, rng):
    """An all-reduce / reduce-scatter / all-gather between the rooted calls (device buffers, out of
    place or in place as coll_workers.coll_rank lays them out, offset / recv_offset included), checked
    the same way.  An all-reduce's tail: elements past the n chunks (count = n * c + tail), which keep
    this rank's input; special: f32 / f64 special values among the inputs.  Out of place the send must
    come back unchanged; grid_calls: the calls this one added to the communicator's read_grid_calls."""
    import hip_rt
    import oracle_api as O
    coll, dtype, op, c = case["coll"], case["dtype"], case.get("op", "sum"), case["count"]
    inplace, seed, (off, roff) = case.get("inplace", False), case.get("seed", 1), CW.offsets(case, rank)
    code, npd = O.DTYPES[dtype]
    esz = np.dtype(npd).itemsize
    tail = case.get("tail", 0) if coll == "ar" else 0
    ns = n * c + tail if coll in ("rs", "ar") else c
    nr = n * c + tail if coll in ("ag", "ar") else c
    mine = rank * c * esz if coll != "ar" else 0
    big = max(ns, nr) * esz
    if inplace:
        whole = hip_rt.DeviceBuffer(big + off + GUARD)
        bufs = [whole]
        send = hip_rt.View(whole, off + (mine if coll == "ag" else 0), ns * esz)
        recv = hip_rt.View(whole, off + (mine if coll == "rs" else 0), nr * esz)
        guard = hip_rt.View(whole, off + big, GUARD)
    else:
        sbuf, rbuf = hip_rt.DeviceBuffer(ns * esz + off), hip_rt.DeviceBuffer(nr * esz + roff + GUARD)
        bufs = [sbuf, rbuf]
        send, recv = hip_rt.View(sbuf, off, ns * esz), hip_rt.View(rbuf, roff, nr * esz)
        guard = hip_rt.View(rbuf, roff + nr * esz, GUARD)
        rbuf.fill_byte(FILL)
    xs = make_inputs(n, ns, dtype, seed, case.get("special", False))
    exp = CW.expected(coll, xs, rank, dtype, op)
    send.upload(xs[rank])
    guard.upload(np.full(GUARD, FILL, np.uint8))
    hip_rt.sync()
    if barrier is not None:
        barrier.wait(120)
    if case.get("skew_ms"):
        time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
    t0 = time.time()
    grid0 = comm.info()["read_grid_calls"]
    rc = CW.call(comm, coll, send.ptr, recv.ptr, c if coll != "ar" else ns, code, O.OPS[op], stream.handle)
    bad, first, detail, algos = -1, -1, "", []
    if rc == 0:
        stream.sync()
        algos.append(comm.info()["last_algo"])
        got = recv.download(npd, nr)
        bad, first = compare(got, exp, dtype, coll != "ag" and op in ("sum", "prod"))
        if bad:
            detail = f"got {got[first]!r} expected {exp[first]!r}"
        bad += int((guard.download(np.uint8, GUARD) != FILL).sum())
        if not inplace:  # the send is only read
            bad += compare(send.download(npd, ns), xs[rank], dtype, False)[0]
    res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos, "secs": time.time() - t0,
           "grid_calls": comm.info()["read_grid_calls"] - grid0}
    res.update(_info_fields(comm))
    for b in bufs:
        b.free()
    return res


def rooted_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked (see _rooted_case / _unrooted_case)."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        stream = hip_rt.Stream()
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            rng = np.random.default_rng(case.get("seed", 1) * 97 + rank)
            run = _rooted_case if case["coll"] in ("bc", "rd") else _unrooted_case
            results.append(run(comm, case, rank, n, stream, barrier, rng))
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def compose_rank(rank, n, port, env, algo, count, rounds, out_q, barrier=None):
    """Reduce(root), then Broadcast(root) of its result, against this rank's own all_reduce of the
    same inputs (and the oracle's), bit for bit; count % n == 0; the root moves every round, new
    inputs every round.  Non-roots pass NULL for the buffers their role does not use."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(algo)
        st = hip_rt.Stream()
        nb = count * 4
        src, red, out_b, ref = (hip_rt.DeviceBuffer(nb) for _ in range(4))
        out = {"rcs": [], "root_bad_vs_allreduce": [], "bad_vs_allreduce": [], "bad_vs_oracle": [], "algos": []}
        for k in range(rounds):
            root = (k + 1) % n
            xs = O.random_inputs(n, count, "f32", seed=8000 + 31 * k)
            exp = O.allreduce(xs, "f32", "sum")[rank]
            src.upload(xs[rank])
            red.fill_byte(0)
            out_b.fill_byte(0)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            is_root = rank == root
            rcs = [comm.reduce(src.ptr, red.ptr if is_root else None, count, M.ncclFloat, M.ncclSum, root, st.handle)]
            a1 = comm.info()["last_algo"]
            rcs.append(comm.broadcast(red.ptr if is_root else None, out_b.ptr, count, M.ncclFloat, root, st.handle))
            a2 = comm.info()["last_algo"]
            rcs.append(comm.all_reduce(src.ptr, ref.ptr, count, M.ncclFloat, M.ncclSum, st.handle))
            st.sync()
            whole = ref.download(np.float32, count)
            got = out_b.download(np.float32, count)
            mid = red.download(np.float32, count)
            out["rcs"].append(rcs)
            out["algos"].append((a1, a2, comm.info()["last_algo"]))
            # the Reduce's own result on the root; a non-root's (unused, never passed) buffer stays 0
            out["root_bad_vs_allreduce"].append(int((mid.view(np.uint32) != whole.view(np.uint32)).sum()) if is_root
                                                else int((mid.view(np.uint32) != 0).sum()))
            out["bad_vs_allreduce"].append(int((got.view(np.uint32) != whole.view(np.uint32)).sum()))
            out["bad_vs_oracle"].append(compare(got, exp, "f32", True)[0])
        out.update(_info_fields(comm))
        for b in (src, red, out_b, ref):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def consumer_rank(rank, n, port, env, coll, count, rounds, out_q, barrier=None):
    """gpu_workers.cached_consumer_rank's shape for the rooted kernels' pushes: the buffer the call
    fills -- every rank's recv for "bc", the root's for "rd" -- is first read by an ordinary kernel
    (its lines sit in this GPU's L2), then the call (the peers push their chunks into it), and an
    ordinary kernel copies it with plain loads right behind the call on the same stream
    (MINI_NCCL_BLOCKING=0: no host wait in between).  New data and another root every round."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        import rooted_ref
        use_rank_device(rank)
        K = testkern()
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        nb = count * 4
        send, recv, seen, word = hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(256)
        recv.fill_byte(0)
        bad, rcs, algos = [], [], []
        for c in range(rounds):
            root = c % n
            reads = coll == "bc" or rank == root
            xs = O.random_inputs(n, count, "f32", seed=6000 + 17 * c)
            send.upload(xs[rank])
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            if reads:
                hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), nb, ctypes.c_void_p(word.ptr),
                                                ctypes.c_void_p(st.handle)), "touch")
            if coll == "bc":
                rc = comm.broadcast(send.ptr, recv.ptr, count, M.ncclFloat, root, st.handle)
            else:
                rc = comm.reduce(send.ptr, recv.ptr if rank == root else None, count, M.ncclFloat, M.ncclSum, root, st.handle)
            if reads:
                hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), nb,
                                               ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            if reads:
                exp = xs[root] if coll == "bc" else rooted_ref.reduce_expect(xs, "f32", "sum")
                bad.append(compare(seen.download(np.float32, count), exp, "f32", coll == "rd")[0])
            else:
                bad.append(0)
        out = {"rcs": rcs, "bad": bad, "algos": algos}
        out.update(_info_fields(comm))
        for b in (send, recv, seen, word):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def errors_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """The calls the library must refuse, on device buffers under the read schedule (n = 2):
      root     -- the ranks disagree on the root: ncclInvalidUsage on every rank, not a hang;
      kinds    -- rank 0 calls Broadcast where rank 1 calls Reduce: ncclInvalidUsage;
      range    -- root = n, root = -1: ncclInvalidArgument;
      null     -- a buffer the rank's role needs is NULL: ncclInvalidArgument (every rank passes a
                  refusable call: recv / send NULL everywhere, then the root lacking its own side
                  while the other rank lacks its);
      overlap  -- send and recv overlap on the root without being equal (each rank names itself the
                  root, so each is refused before anything is negotiated): ncclInvalidArgument;
      dtype    -- an unsupported datatype: ncclInternalError.
    Then the communicator's next valid calls succeed and are right."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        import rooted_ref
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        c = 4099
        a, b = hip_rt.DeviceBuffer(c * 4 + 64), hip_rt.DeviceBuffer(c * 4)
        xs = O.random_inputs(n, c, "f32", seed=77)
        a.upload(xs[rank])
        b.fill_byte(0)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        F, S, h = M.ncclFloat, M.ncclSum, st.handle
        rcs = []
        if scenario == "root":
            rcs.append(comm.broadcast(a.ptr, b.ptr, c, F, rank, h))
            rcs.append(comm.reduce(a.ptr, b.ptr, c, F, S, rank, h))
        elif scenario == "kinds":
            rcs.append(comm.broadcast(a.ptr, b.ptr, c, F, 0, h) if rank == 0 else comm.reduce(a.ptr, b.ptr, c, F, S, 0, h))
        elif scenario == "range":
            rcs += [comm.broadcast(a.ptr, b.ptr, c, F, n, h), comm.broadcast(a.ptr, b.ptr, c, F, -1, h),
                    comm.reduce(a.ptr, b.ptr, c, F, S, n, h), comm.reduce(a.ptr, b.ptr, c, F, S, -1, h)]
        elif scenario == "null":
            root = 0
            rcs += [comm.broadcast(a.ptr, None, c, F, root, h), comm.reduce(None, b.ptr, c, F, S, root, h),
                    # the root lacks the side only it needs; the other rank lacks its own
                    comm.broadcast(None, b.ptr if rank == root else None, c, F, root, h),
                    comm.reduce(a.ptr if rank == root else None, None, c, F, S, root, h)]
        elif scenario == "overlap":
            rcs += [comm.broadcast(a.ptr, a.ptr + 8, c, F, rank, h), comm.reduce(a.ptr + 8, a.ptr, c, F, S, rank, h)]
        else:
            rcs += [comm.broadcast(a.ptr, b.ptr, c, M.ncclUint64, 0, h), comm.reduce(a.ptr, b.ptr, c, M.ncclInt8, S, 0, h)]
        out = {"rcs": rcs, "async_after": comm.async_error()}
        # the communicator is still usable: a Broadcast from rank 1, then a Reduce to rank 0, checked
        a.upload(xs[rank])
        hip_rt.sync()
        rc1 = comm.broadcast(a.ptr if rank == 1 else None, b.ptr, c, F, 1, h)
        st.sync()
        got1 = b.download(np.float32, c)
        rc2 = comm.reduce(a.ptr, b.ptr if rank == 0 else None, c, F, S, 0, h)
        st.sync()
        got2 = b.download(np.float32, c)
        out["next_rc"] = [rc1, rc2]
        out["next_bad"] = -1
        if rc1 == 0 and rc2 == 0:
            exp2 = rooted_ref.reduce_expect(xs, "f32", "sum") if rank == 0 else xs[1]  # rank 1's b: untouched
            out["next_bad"] = compare(got1, xs[1], "f32", False)[0] + compare(got2, exp2, "f32", rank == 0)[0]
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
