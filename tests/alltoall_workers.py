"""Rank processes for the ncclAllToAll GPU tests (one process = one rank; placement, spawning and
the consumer kernels are tests/gpu_workers.py's, the five other collectives' cases
tests/rooted_workers.py's).

The expected result is the permutation itself: block r of rank q's recv is block q of rank r's send.
Buffers are seeded random BYTES -- block(seed, r, q) is block q of rank r's send, so every rank can
compute the blocks it sends and the blocks it must receive without the others' whole buffers -- and
are compared as bytes.  After every call: 256 guard bytes past recv unchanged, the send unchanged.
"""
import ctypes
import os
import time
import traceback

import numpy as np

import rooted_workers as RW
from coll_workers import GUARD, _info_fields, offsets
from gpu_workers import testkern, use_rank_device

FILL = 0xAB


def block(seed, r, q, nbytes):
    """Block q of rank r's send: seeded random bytes (NaN payloads, denormals, every bit pattern)."""
    return np.frombuffer(np.random.default_rng([seed, r, q]).bytes(nbytes), np.uint8)


def my_send(seed, rank, n, bb):
    return np.concatenate([block(seed, rank, q, bb) for q in range(n)])


def my_expect(seed, rank, n, bb):
    return np.concatenate([block(seed, r, rank, bb) for r in range(n)])


def _differ(got, exp):
    d = np.flatnonzero(got != exp)
    return int(d.size), (int(d[0]) if d.size else -1)


def _a2a_case(comm, case, rank, n, stream, barrier, rng):
    """One all-to-all case: dtype, count (elements per block), algo, seed, calls (new bytes every
    call), offset / recv_offset (bytes: a misaligned base, or a per-rank list of them; recv_offset
    defaults to offset), mem / recv_mem (device / pinned / pageable, or a per-rank list), skew_ms."""
    import hip_rt
    import oracle_api as O
    dtype, c, seed, (off, roff) = case["dtype"], case["count"], case.get("seed", 1), offsets(case, rank)
    code, npd = O.DTYPES[dtype]
    bb = c * np.dtype(npd).itemsize
    nb = n * bb
    mem_s = RW._placement(case, "mem", "device", rank)
    mem_r = RW._placement(case, "recv_mem", mem_s, rank)
    sbuf, rbuf = hip_rt.buffer(mem_s, nb + off), hip_rt.buffer(mem_r, nb + roff + GUARD)
    send, recv, guard = hip_rt.View(sbuf, off, nb), hip_rt.View(rbuf, roff, nb), hip_rt.View(rbuf, roff + nb, GUARD)
    bad, first, detail, rc, algos = 0, -1, "", 0, []
    t0 = time.time()
    for k in range(case.get("calls", 1)):
        mine, exp = my_send(seed + 1000 * k, rank, n, bb), my_expect(seed + 1000 * k, rank, n, bb)
        rbuf.fill_byte(FILL)
        send.upload(mine)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        if case.get("skew_ms"):
            time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
        rc = comm.all_to_all(send.ptr, recv.ptr, c, code, stream.handle)
        if rc != 0:
            bad = -1
            break
        stream.sync()
        algos.append(comm.info()["last_algo"])
        got = recv.download(np.uint8, nb)
        b, f = _differ(got, exp)
        if b and not bad:
            first, detail = f, f"call {k}: byte {f} (block {f // bb}) got {got[f]} expected {exp[f]}"
        b += int((guard.download(np.uint8, GUARD) != FILL).sum())   # nothing written past recv
        b += _differ(send.download(np.uint8, nb), mine)[0]           # the send is only read
        bad += b
    res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos, "secs": time.time() - t0}
    res.update(_info_fields(comm))
    sbuf.free()
    rbuf.free()
    return res


def a2a_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked: coll "a2a" (the default) here, "bc" /
    "rd" / "ar" / "rs" / "ag" as rooted_workers.rooted_rank runs them."""
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
            coll = case.get("coll", "a2a")
            run = _a2a_case if coll == "a2a" else RW._rooted_case if coll in ("bc", "rd") else RW._unrooted_case
            results.append(run(comm, case, rank, n, stream, barrier, rng))
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def transpose_twice_rank(rank, n, port, env, algo, count, rounds, out_q, barrier=None):
    """Two all-to-alls in a row, the recv of the first fed as the send of the second into a third
    buffer: a transpose applied twice returns every rank's original buffer.  New bytes every round."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(algo)
        st = hip_rt.Stream()
        bb = count * 4
        nb = n * bb
        a, b, c = (hip_rt.DeviceBuffer(nb + GUARD) for _ in range(3))
        out = {"rcs": [], "bad_mid": [], "bad_back": [], "bad_guard": [], "algos": []}
        for k in range(rounds):
            mine, exp = my_send(9000 + k, rank, n, bb), my_expect(9000 + k, rank, n, bb)
            for buf in (a, b, c):
                buf.fill_byte(FILL)
            a.upload(mine)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            rcs = [comm.all_to_all(a.ptr, b.ptr, count, M.ncclFloat, st.handle)]
            a1 = comm.info()["last_algo"]
            rcs.append(comm.all_to_all(b.ptr, c.ptr, count, M.ncclFloat, st.handle))
            st.sync()
            out["rcs"].append(rcs)
            out["algos"].append((a1, comm.info()["last_algo"]))
            out["bad_mid"].append(_differ(b.download(np.uint8, nb), exp)[0])
            out["bad_back"].append(_differ(c.download(np.uint8, nb), mine)[0] + _differ(a.download(np.uint8, nb), mine)[0])
            out["bad_guard"].append(sum(int((x.download(np.uint8, GUARD, nb) != FILL).sum()) for x in (a, b, c)))
        out.update(_info_fields(comm))
        for buf in (a, b, c):
            buf.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def consumer_rank(rank, n, port, env, count, rounds, out_q, barrier=None):
    """gpu_workers.cached_consumer_rank's shape for exchange_push's pushes: recv is first read by an
    ordinary kernel on the call's stream (its lines sit in this GPU's L2), then the all-to-all -- the
    peers push their blocks into this recv -- and an ordinary kernel copies recv with plain loads
    right behind the call on the same stream (MINI_NCCL_BLOCKING=0: no host wait in between).  New
    bytes every round."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        K = testkern()
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        bb = count * 4
        nb = n * bb
        send, recv, seen, word = hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(nb), hip_rt.DeviceBuffer(256)
        recv.fill_byte(0)
        bad, rcs, algos = [], [], []
        for k in range(rounds):
            mine, exp = my_send(6000 + k, rank, n, bb), my_expect(6000 + k, rank, n, bb)
            send.upload(mine)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), nb, ctypes.c_void_p(word.ptr),
                                            ctypes.c_void_p(st.handle)), "touch")
            rc = comm.all_to_all(send.ptr, recv.ptr, count, M.ncclFloat, st.handle)
            hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), nb,
                                           ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            bad.append(_differ(seen.download(np.uint8, nb), exp)[0])
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
      overlap  -- the byte ranges overlap partly, either way round: ncclInvalidArgument;
      same     -- send == recv (there is no in-place form): ncclInvalidArgument;
      null     -- a NULL sendbuff, a NULL recvbuff: ncclInvalidArgument;
      dtype    -- ncclInt8: ncclInternalError;
      kinds    -- rank 0 calls ncclAllToAll where rank 1 calls ncclAllGather with the same count:
                  ncclInvalidUsage on both, not a hang.
    Then mncclCommGetAsyncError is 0 and the communicator's next two valid calls are exact."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        comm.set_algo(M.ALGO_READ)
        st = hip_rt.Stream()
        c = 4099
        bb = c * 4
        nb = n * bb
        a, b = hip_rt.DeviceBuffer(nb + 64), hip_rt.DeviceBuffer(nb + GUARD)
        a.upload(my_send(70, rank, n, bb))
        b.fill_byte(FILL)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        F, h = M.ncclFloat, st.handle
        if scenario == "overlap":
            rcs = [comm.all_to_all(a.ptr, a.ptr + 8, c, F, h), comm.all_to_all(a.ptr + 16, a.ptr, c, F, h),
                   comm.all_to_all(a.ptr + nb - 4, a.ptr, c, F, h)]  # the last word of one is the first of the other
        elif scenario == "same":
            rcs = [comm.all_to_all(a.ptr, a.ptr, c, F, h), comm.all_to_all(b.ptr, b.ptr, 1, F, h)]
        elif scenario == "null":
            rcs = [comm.all_to_all(None, b.ptr, c, F, h), comm.all_to_all(a.ptr, None, c, F, h)]
        elif scenario == "dtype":
            rcs = [comm.all_to_all(a.ptr, b.ptr, c, M.ncclInt8, h)]
        else:
            rcs = [comm.all_to_all(a.ptr, b.ptr, c, F, h) if rank == 0 else comm.all_gather(a.ptr, b.ptr, c, F, h)]
        st.sync()
        out = {"rcs": rcs, "async_after": comm.async_error()}
        # nothing was launched: b still holds its fill
        out["touched"] = int((b.download(np.uint8, nb + GUARD) != FILL).sum())
        # the communicator is still usable: two all-to-alls with fresh bytes, checked
        out["next_rc"], out["next_bad"] = [], 0
        for k in range(2):
            mine, exp = my_send(71 + k, rank, n, bb), my_expect(71 + k, rank, n, bb)
            a.upload(mine)
            hip_rt.sync()
            rc = comm.all_to_all(a.ptr, b.ptr, c, F, h)
            st.sync()
            out["next_rc"].append(rc)
            out["next_bad"] += _differ(b.download(np.uint8, nb), exp)[0] if rc == 0 else 1
            out["next_bad"] += int((b.download(np.uint8, GUARD, nb) != FILL).sum())
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
