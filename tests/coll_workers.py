"""Rank processes for the ncclReduceScatter / ncclAllGather GPU tests (one process = one rank;
placement, spawning and comparison are tests/gpu_workers.py's).

Expected values, computed in-process from the same seeded inputs: a reduce-scatter's rank r holds
chunk r of the oracle's ring fold (the all-reduce's bits), an all-gather's every rank the
concatenation of the ranks' inputs, an all-reduce the oracle's ring all-reduce.
"""
import ctypes
import os
import time
import traceback

import numpy as np

import gpu_workers as GW
from gpu_workers import compare, make_inputs, testkern, use_rank_device

GUARD = 256  # bytes past every recv, filled before the call and checked after it


def expected(coll, xs, rank, dtype, op):
    import oracle_api as O
    n = len(xs)
    if coll == "ar":
        return O.allreduce(xs, dtype, op)[rank]
    if coll == "rs":
        c = xs[0].size // n
        return O.ring_fold(xs, dtype, op)[rank * c:(rank + 1) * c]
    return np.concatenate(xs)


def _info_fields(comm):
    ci = comm.info()
    return {"last_algo": ci["last_algo"], "ipc_open_failures": ci["ipc_open_failures"],
            "read_map_failures": ci["read_map_failures"], "async": comm.async_error()}


def per_rank(v, rank):
    """A case's value for this rank: the value itself, or entry rank of a per-rank list."""
    return v[rank % len(v)] if isinstance(v, (list, tuple)) else v


def offsets(case, rank):
    """(offset, recv_offset) of this rank in bytes: each a value or a per-rank list; recv_offset
    defaults to offset (in place the one offset serves both buffers)."""
    off = case.get("offset", 0)
    return per_rank(off, rank), per_rank(case.get("recv_offset", off), rank)


def call(comm, coll, send_ptr, recv_ptr, count, code, opc, stream):
    if coll == "rs":
        return comm.reduce_scatter(send_ptr, recv_ptr, count, code, opc, stream)
    if coll == "ag":
        return comm.all_gather(send_ptr, recv_ptr, count, code, stream)
    return comm.all_reduce(send_ptr, recv_ptr, count, code, opc, stream)


def coll_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked.  A case: coll ("rs" / "ag" / "ar"),
    dtype, op, count (elements per rank; an all-reduce runs over n * count), inplace, algo, seed and
    optionally calls (new inputs every call), special (f32 / f64 special values), offset / recv_offset
    (bytes: a misaligned base, or a per-rank list of them; recv_offset defaults to offset), mem /
    recv_mem (device / pinned / pageable, or a per-rank list), skew_ms."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        stream = hip_rt.Stream()
        results = []
        for case in cases:
            coll, dtype, op, c = case["coll"], case["dtype"], case.get("op", "sum"), case["count"]
            inplace, seed, (off, roff) = case.get("inplace", False), case.get("seed", 1), offsets(case, rank)
            comm.set_algo(case["algo"])
            code, npd = O.DTYPES[dtype]
            esz = np.dtype(npd).itemsize
            # elements in send / recv; where this rank's one-chunk buffer sits in the other (in place)
            ns = n * c if coll in ("rs", "ar") else c
            nr = n * c if coll in ("ag", "ar") else c
            mine = rank * c * esz if coll != "ar" else 0

            def placement(key, dflt):
                m = case.get(key, dflt)
                return m[rank % len(m)] if isinstance(m, (list, tuple)) else m
            big = max(ns, nr) * esz
            if inplace:
                whole = hip_rt.buffer(placement("mem", "device"), big + off + GUARD)
                send = hip_rt.View(whole, off + (mine if coll == "ag" else 0), ns * esz)
                recv = hip_rt.View(whole, off + (mine if coll == "rs" else 0), nr * esz)
                guard = hip_rt.View(whole, off + big, GUARD)
            else:
                sbuf = hip_rt.buffer(placement("mem", "device"), ns * esz + off)
                rbuf = hip_rt.buffer(placement("recv_mem", placement("mem", "device")), nr * esz + roff + GUARD)
                send, recv = hip_rt.View(sbuf, off, ns * esz), hip_rt.View(rbuf, roff, nr * esz)
                guard = hip_rt.View(rbuf, roff + nr * esz, GUARD)
                rbuf.fill_byte(0xAB)
            bad, first, detail, rc, algos = 0, -1, "", 0, []
            rng = np.random.default_rng(seed * 97 + rank)
            t0 = time.time()
            for k in range(case.get("calls", 1)):
                xs = make_inputs(n, ns, dtype, seed + 1000 * k, case.get("special", False))
                exp = expected(coll, xs, rank, dtype, op)
                send.upload(xs[rank])
                guard.upload(np.full(GUARD, 0xAB, np.uint8))
                hip_rt.sync()
                if barrier is not None:
                    barrier.wait(120)
                if case.get("skew_ms"):
                    time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
                rc = call(comm, coll, send.ptr, recv.ptr, c if coll != "ar" else ns, code, O.OPS[op], stream.handle)
                if rc != 0:
                    bad = -1
                    break
                stream.sync()
                algos.append(comm.info()["last_algo"])
                got = recv.download(npd, nr)
                b, f = compare(got, exp, dtype, coll != "ag" and op in ("sum", "prod"))
                b += int((guard.download(np.uint8, GUARD) != 0xAB).sum())  # nothing written past recv
                if b and not bad:
                    first, detail = f, f"call {k}: got {got[f]!r} expected {exp[f]!r}"
                bad += b
            res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos,
                   "secs": time.time() - t0}
            res.update(_info_fields(comm))
            results.append(res)
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


def compose_rank(rank, n, port, env, algo, count, calls, out_q, barrier=None):
    """reduce_scatter then all_gather, in place on one buffer of n * count floats, against this
    rank's own all_reduce of the same inputs (and the oracle's), bit for bit; new inputs every call."""
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
        nb, cb = n * count * 4, count * 4
        buf, src, ref = hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb)
        out = {"rcs": [], "bad_vs_allreduce": [], "bad_vs_oracle": [], "algos": []}
        for k in range(calls):
            xs = O.random_inputs(n, n * count, "f32", seed=7000 + 31 * k)
            exp = O.allreduce(xs, "f32", "sum")[rank]
            buf.upload(xs[rank])
            src.upload(xs[rank])
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            rcs = [comm.reduce_scatter(buf.ptr, buf.ptr + rank * cb, count, M.ncclFloat, M.ncclSum, st.handle)]
            a1 = comm.info()["last_algo"]
            rcs.append(comm.all_gather(buf.ptr + rank * cb, buf.ptr, count, M.ncclFloat, st.handle))
            a2 = comm.info()["last_algo"]
            rcs.append(comm.all_reduce(src.ptr, ref.ptr, n * count, M.ncclFloat, M.ncclSum, st.handle))
            st.sync()
            got, whole = buf.download(np.float32, n * count), ref.download(np.float32, n * count)
            out["rcs"].append(rcs)
            out["algos"].append((a1, a2, comm.info()["last_algo"]))
            out["bad_vs_allreduce"].append(int((got.view(np.uint32) != whole.view(np.uint32)).sum()))
            out["bad_vs_oracle"].append(compare(got, exp, "f32", True)[0])
        out.update(_info_fields(comm))
        for b in (buf, src, ref):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def gather_consumer_rank(rank, n, port, env, count, calls, out_q, barrier=None):
    """gpu_workers.cached_consumer_rank's shape for gather_push's pushes: recv is first read by an
    ordinary kernel (its lines sit in this GPU's L2), then the all-gather -- the peers push their
    chunks into this recv -- and an ordinary kernel copies recv with plain loads right behind the
    call on the same stream (MINI_NCCL_BLOCKING=0: no host wait in between).  New data every call."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        use_rank_device(rank)
        K = testkern()
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        cb, nb = count * 4, n * count * 4
        send, recv, seen = hip_rt.DeviceBuffer(cb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb)
        word = hip_rt.DeviceBuffer(256)
        recv.fill_byte(0)
        bad, rcs, algos = [], [], []
        for c in range(calls):
            inplace = c % 3 == 2
            xs = O.random_inputs(n, count, "f32", seed=5000 + 17 * c)
            exp = np.concatenate(xs)
            src_ptr = recv.ptr + rank * cb if inplace else send.ptr
            (recv if inplace else send).upload(xs[rank], rank * cb if inplace else 0)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), nb, ctypes.c_void_p(word.ptr),
                                            ctypes.c_void_p(st.handle)), "touch")
            rc = comm.all_gather(src_ptr, recv.ptr, count, M.ncclFloat, st.handle)
            hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), nb,
                                           ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            got = seen.download(np.float32, n * count)
            bad.append(compare(got, exp, "f32", False)[0])
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
    """The calls the library must refuse, on device buffers under the read schedule:
      overlap  -- send and recv overlap without being in place: ncclInvalidArgument on every rank,
                  nothing launched, and the next valid call succeeds and is right;
      counts   -- the ranks pass different counts: ncclInvalidUsage on every rank, not a hang;
      kinds    -- rank 0 calls reduce_scatter where the others call all_gather: ncclInvalidUsage;
      dtype    -- an unsupported datatype: ncclInternalError, communicator still usable."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        import oracle_api as O
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        c = 1024
        big, small = hip_rt.DeviceBuffer(n * c * 4 + 64), hip_rt.DeviceBuffer(c * 4)
        xs = O.random_inputs(n, n * c, "f32", seed=99)
        big.upload(xs[rank])
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        rcs = []
        if scenario == "overlap":
            # recv starts 8 bytes past where in place would put it: overlaps send, not in place
            rcs.append(comm.reduce_scatter(big.ptr, big.ptr + rank * c * 4 + 8, c, M.ncclFloat, M.ncclSum, st.handle))
            rcs.append(comm.all_gather(big.ptr + rank * c * 4 + 8, big.ptr, c, M.ncclFloat, st.handle))
        elif scenario == "counts":
            rcs.append(comm.reduce_scatter(big.ptr, small.ptr, c - rank, M.ncclFloat, M.ncclSum, st.handle))
        elif scenario == "kinds":
            if rank == 0:
                rcs.append(comm.reduce_scatter(big.ptr, small.ptr, c, M.ncclFloat, M.ncclSum, st.handle))
            else:
                rcs.append(comm.all_gather(small.ptr, big.ptr, c, M.ncclFloat, st.handle))
        else:
            rcs.append(comm.reduce_scatter(big.ptr, small.ptr, c, M.ncclInt8, M.ncclSum, st.handle))
            rcs.append(comm.all_gather(small.ptr, big.ptr, c, M.ncclUint64, st.handle))
        out = {"rcs": rcs, "async_after": comm.async_error()}
        # the communicator is still usable: a valid call, checked
        big.upload(xs[rank])
        hip_rt.sync()
        rc = comm.reduce_scatter(big.ptr, small.ptr, c, M.ncclFloat, M.ncclSum, st.handle)
        st.sync()
        got = small.download(np.float32, c)
        out["next_rc"] = rc
        out["next_bad"] = compare(got, expected("rs", xs, rank, "f32", "sum"), "f32", True)[0] if rc == 0 else -1
        out.update(_info_fields(comm))
        big.free()
        small.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
