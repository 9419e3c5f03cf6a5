"""Rank processes for the ncclAllToAllv GPU tests (one process = one rank; placement, spawning and
the consumer kernels are tests/gpu_workers.py's, the six other collectives' cases
tests/alltoall_workers.py's and tests/rooted_workers.py's).

The expected result is the permutation itself: elements [sd[r][q], +C[r][q]) of rank r's send are
elements [rd[q][r], +C[r][q]) of rank q's recv.  block(seed, r, q) is the block rank r sends to rank
q -- seeded random BYTES, so every rank computes what it sends and what it must receive without the
others' buffers -- compared as bytes.  A recv starts as FILL bytes: after every call the gaps between
its blocks and the 256 guard bytes behind it are unchanged, and so is the send.
"""
import ctypes
import os
import time
import traceback

import numpy as np

import alltoall_workers as AW
import rooted_workers as RW
from coll_workers import GUARD, _info_fields, offsets
from gpu_workers import testkern, use_rank_device
from sim_alltoallv_api import displacements

FILL = AW.FILL
block = AW.block
_differ = AW._differ


class Shape:
    """One call's matrix and displacements, as every rank derives them from the case: C[r][q]
    elements from r to q; mode "contig" / "reversed" / "gaps" (sim_alltoallv_api.displacements), or
    explicit per-rank lists case["sd"] / case["rd"]."""

    def __init__(self, case, n, esz):
        self.C = np.array(case["C"], dtype=np.int64).reshape(n, n)
        self.n, self.esz = n, esz
        mode = case.get("mode", "contig")
        self.sd = case["sd"] if "sd" in case else [displacements(self.C[r, :], mode)[0] for r in range(n)]
        self.rd = case["rd"] if "rd" in case else [displacements(self.C[:, r], mode)[0] for r in range(n)]

    def send_bytes(self, r):
        return max([(self.sd[r][q] + int(self.C[r, q])) * self.esz for q in range(self.n)] + [self.esz])

    def recv_bytes(self, r):
        return max([(self.rd[r][q] + int(self.C[q, r])) * self.esz for q in range(self.n)] + [self.esz])

    def my_send(self, seed, r):
        x = np.frombuffer(np.random.default_rng([seed, r, 999]).bytes(self.send_bytes(r)), np.uint8).copy()
        for q in range(self.n):
            c, at = int(self.C[r, q]) * self.esz, self.sd[r][q] * self.esz
            x[at:at + c] = block(seed, r, q, c)
        return x

    def my_expect(self, seed, r, base=None):
        x = np.full(self.recv_bytes(r), FILL, np.uint8) if base is None else base.copy()
        for q in range(self.n):
            c, at = int(self.C[q, r]) * self.esz, self.rd[r][q] * self.esz
            x[at:at + c] = block(seed, q, r, c)
        return x

    def args(self, r):
        return ([int(v) for v in self.C[r, :]], self.sd[r], [int(v) for v in self.C[:, r]], self.rd[r])


def _v_case(comm, case, rank, n, stream, barrier, rng):
    """One ncclAllToAllv case: dtype, C, mode / sd / rd, algo, seed, calls (new bytes every call),
    offset / recv_offset (bytes: a misaligned base, or a per-rank list), mem / recv_mem (device /
    pinned / pageable, or a per-rank list), null_ranks (they pass NULL for both buffers: their row and
    column of C are zero), skew_ms, vs_a2a (uniform contiguous C: ncclAllToAll on the same send into a
    second recv must give the same bytes)."""
    import hip_rt
    import oracle_api as O
    dtype, seed, (off, roff) = case["dtype"], case.get("seed", 1), offsets(case, rank)
    code, npd = O.DTYPES[dtype]
    sh = Shape(case, n, np.dtype(npd).itemsize)
    null = rank in case.get("null_ranks", ())
    sb, rb = sh.send_bytes(rank), sh.recv_bytes(rank)
    mem_s = RW._placement(case, "mem", "device", rank)
    mem_r = RW._placement(case, "recv_mem", mem_s, rank)
    sbuf, rbuf = hip_rt.buffer(mem_s, sb + off), hip_rt.buffer(mem_r, rb + roff + GUARD)
    send, recv, guard = hip_rt.View(sbuf, off, sb), hip_rt.View(rbuf, roff, rb), hip_rt.View(rbuf, roff + rb, GUARD)
    r2 = hip_rt.DeviceBuffer(rb) if case.get("vs_a2a") else None
    sc, sd, rc_, rd = sh.args(rank)
    bad, first, detail, rc, algos = 0, -1, "", 0, []
    t0 = time.time()
    for k in range(case.get("calls", 1)):
        mine, exp = sh.my_send(seed + 1000 * k, rank), sh.my_expect(seed + 1000 * k, rank)
        rbuf.fill_byte(FILL)
        send.upload(mine)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        if case.get("skew_ms"):
            time.sleep(float(rng.uniform(0, case["skew_ms"])) / 1000.0)
        rc = comm.all_to_all_v(None if null else send.ptr, sc, sd, None if null else recv.ptr, rc_, rd, code, stream.handle)
        if rc != 0:
            bad = -1
            break
        stream.sync()
        algos.append(comm.info()["last_algo"])
        got = recv.download(np.uint8, rb)
        b, f = _differ(got, exp)
        if b and not bad:
            first, detail = f, f"call {k}: byte {f} of recv got {got[f]} expected {exp[f]}"
        b += int((guard.download(np.uint8, GUARD) != FILL).sum())   # nothing written past recv
        b += _differ(send.download(np.uint8, sb), mine)[0]           # the send is only read
        if r2 is not None:
            r2.fill_byte(FILL)
            assert comm.all_to_all(send.ptr, r2.ptr, int(sh.C[0, 0]), code, stream.handle) == 0
            stream.sync()
            b += _differ(r2.download(np.uint8, rb), got)[0]
        bad += b
    res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos, "secs": time.time() - t0}
    res.update(_info_fields(comm))
    sbuf.free()
    rbuf.free()
    if r2 is not None:
        r2.free()
    return res


def v_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` on one communicator, every call checked: coll "a2av" (the default) here, "a2a" as
    alltoall_workers, "bc" / "rd" / "ar" / "rs" / "ag" as rooted_workers.rooted_rank runs them."""
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
            coll = case.get("coll", "a2av")
            run = _v_case if coll == "a2av" else AW._a2a_case if coll == "a2a" else \
                RW._rooted_case if coll in ("bc", "rd") else RW._unrooted_case
            results.append(run(comm, case, rank, n, stream, barrier, rng))
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def _open(rank, n, port, env, algo):
    os.environ.update(env)
    os.environ["MINI_NCCL_PORT"] = str(port)
    import hip_rt
    import mini_nccl as M
    use_rank_device(rank)
    comm = M.Comm(n, rank, "127.0.0.1")
    comm.set_algo(algo)
    return hip_rt, M, comm, hip_rt.Stream()


def round_trip_rank(rank, n, port, env, algo, C, rounds, out_q, barrier=None):
    """A call with matrix C (gapped displacements) from a into b, then a call with the roles of send
    and recv exchanged -- b's blocks sent back with the transposed matrix -- into c at a's
    displacements: every block of a is back in c.  New bytes every round."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, algo)
        sh = Shape({"C": C, "mode": "gaps"}, n, 4)
        sb, rb = sh.send_bytes(rank), sh.recv_bytes(rank)
        a, b, c = hip_rt.DeviceBuffer(sb + GUARD), hip_rt.DeviceBuffer(rb + GUARD), hip_rt.DeviceBuffer(sb + GUARD)
        sc, sd, rc_, rd = sh.args(rank)
        out = {"rcs": [], "bad_mid": [], "bad_back": [], "bad_guard": [], "algos": []}
        for k in range(rounds):
            mine, exp = sh.my_send(9000 + k, rank), sh.my_expect(9000 + k, rank)
            for buf in (a, b, c):
                buf.fill_byte(FILL)
            a.upload(mine)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            rcs = [comm.all_to_all_v(a.ptr, sc, sd, b.ptr, rc_, rd, M.ncclFloat, st.handle)]
            a1 = comm.info()["last_algo"]
            rcs.append(comm.all_to_all_v(b.ptr, rc_, rd, c.ptr, sc, sd, M.ncclFloat, st.handle))
            st.sync()
            out["rcs"].append(rcs)
            out["algos"].append((a1, comm.info()["last_algo"]))
            out["bad_mid"].append(_differ(b.download(np.uint8, rb), exp)[0])
            # c: FILL, with every block of a back at its displacement (a's gap bytes never travelled)
            back = np.full(sb, FILL, np.uint8)
            for q in range(n):
                cnt, at = int(sh.C[rank, q]) * 4, sd[q] * 4
                back[at:at + cnt] = mine[at:at + cnt]
            out["bad_back"].append(_differ(c.download(np.uint8, sb), back)[0] + _differ(a.download(np.uint8, sb), mine)[0])
            out["bad_guard"].append(sum(int((x.download(np.uint8, GUARD, m) != FILL).sum())
                                        for x, m in ((a, sb), (b, rb), (c, sb))))
        out.update(_info_fields(comm))
        for buf in (a, b, c):
            buf.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def consumer_rank(rank, n, port, env, C, rounds, out_q, barrier=None):
    """alltoall_workers.consumer_rank's shape for varblock_push's pushes: recv is first read by an
    ordinary kernel on the call's stream (its lines sit in this GPU's L2), then the call -- the peers
    push their blocks into this recv -- and an ordinary kernel copies recv with plain loads right
    behind the call on the same stream (MINI_NCCL_BLOCKING=0: no host wait in between)."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, M_READ)
        K = testkern()
        sh = Shape({"C": C, "mode": "contig"}, n, 4)
        sb, rb = sh.send_bytes(rank), sh.recv_bytes(rank)
        send, recv, seen, word = (hip_rt.DeviceBuffer(x) for x in (sb, rb, rb, 256))
        recv.fill_byte(0)
        sc, sd, rc_, rd = sh.args(rank)
        bad, rcs, algos = [], [], []
        for k in range(rounds):
            mine = sh.my_send(6000 + k, rank)
            exp = sh.my_expect(6000 + k, rank, base=np.zeros(rb, np.uint8))
            send.upload(mine)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), rb, ctypes.c_void_p(word.ptr),
                                            ctypes.c_void_p(st.handle)), "touch")
            rc = comm.all_to_all_v(send.ptr, sc, sd, recv.ptr, rc_, rd, M.ncclFloat, st.handle)
            hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), rb,
                                           ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            bad.append(_differ(seen.download(np.uint8, rb), exp)[0])
        out = {"rcs": rcs, "bad": bad, "algos": algos}
        out.update(_info_fields(comm))
        for b in (send, recv, seen, word):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


M_READ, M_RING = 2, 0


def errors_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """The calls the library must refuse, on device buffers under the read schedule (n = 2):
      null_array -- a NULL sendcounts / sdispls / recvcounts / rdispls: ncclInvalidArgument;
      recv_overlap -- two recv blocks overlap by one element: ncclInvalidArgument;
      send_recv  -- a recv block overlaps a send block, and send == recv: ncclInvalidArgument;
      dtype      -- ncclInt8: ncclInternalError;
      mismatch   -- rank 1 expects one element more from rank 0 than rank 0 sends: ncclInvalidUsage
                    on both ranks;
      kinds      -- rank 0 calls ncclAllToAllv where rank 1 calls ncclAllToAll: ncclInvalidUsage on both.
    Then mncclCommGetAsyncError is 0 and the communicator's next two valid calls are exact."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, M_READ)
        L = M.load()
        c = 4099
        sh = Shape({"C": [[c, c - 7], [c + 5, 3]], "mode": "gaps"}, n, 4)
        sb, rb = sh.send_bytes(rank), sh.recv_bytes(rank)
        a, b = hip_rt.DeviceBuffer(sb + 64), hip_rt.DeviceBuffer(rb + GUARD)
        a.upload(sh.my_send(70, rank))
        b.fill_byte(FILL)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        F, h = M.ncclFloat, st.handle
        sc, sd, rc_, rd = sh.args(rank)
        v = lambda s, r, sc=sc, sd=sd, rc_=rc_, rd=rd, dt=F: comm.all_to_all_v(s, sc, sd, r, rc_, rd, dt, h)
        if scenario == "null_array":
            arr = (ctypes.c_size_t * n)(*sc)
            raw = lambda *p: L.ncclAllToAllv(a.ptr, p[0], p[1], b.ptr, p[2], p[3], F, comm.handle, h)
            rcs = [raw(*[None if i == k else arr for i in range(4)]) for k in range(4)]
        elif scenario == "recv_overlap":
            rcs = [v(a.ptr, b.ptr, rd=[rd[1] + rc_[1] - 1, rd[1]]), v(a.ptr, b.ptr, rd=[rd[0], rd[0]])]
        elif scenario == "send_recv":
            rcs = [v(a.ptr, a.ptr), v(a.ptr, a.ptr + 4 * (sd[0] + sc[0] - 1 - rd[1])),  # one element of overlap
                   v(b.ptr + 8, b.ptr)]
        elif scenario == "dtype":
            rcs = [v(a.ptr, b.ptr, dt=M.ncclInt8)]
        elif scenario == "mismatch":
            rcs = [v(a.ptr, b.ptr, rc_=[rc_[0] + 1, rc_[1]]) if rank == 1 else v(a.ptr, b.ptr)]
        else:
            rcs = [v(a.ptr, b.ptr) if rank == 0 else comm.all_to_all(a.ptr, b.ptr, 3, F, h)]
        st.sync()
        out = {"rcs": rcs, "async_after": comm.async_error()}
        out["touched"] = int((b.download(np.uint8, rb + GUARD) != FILL).sum())  # nothing was launched
        out["next_rc"], out["next_bad"] = [], 0
        for k in range(2):
            mine, exp = sh.my_send(71 + k, rank), sh.my_expect(71 + k, rank)
            a.upload(mine)
            hip_rt.sync()
            rc = v(a.ptr, b.ptr)
            st.sync()
            out["next_rc"].append(rc)
            out["next_bad"] += _differ(b.download(np.uint8, rb), exp)[0] if rc == 0 else 1
            out["next_bad"] += int((b.download(np.uint8, GUARD, rb) != FILL).sum())
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def graph_rank(rank, n, port, env, algo, C, replays, out_q, barrier=None):
    """lifecycle_workers.graph_rank's pattern: ONE call captured into a HIP graph (the buffers hold a
    first seed's data, which no replay expects), replayed with new seeded inputs and recv refilled
    before every replay, then one eager call.  Under a forced ring the captured call is refused on
    every rank (the padded fallback's stage cannot be allocated inside a capture): the graph is
    empty, and the eager call still runs."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, algo)
        sh = Shape({"C": C, "mode": "gaps"}, n, 4)
        sb, rb = sh.send_bytes(rank), sh.recv_bytes(rank)
        a, b = hip_rt.DeviceBuffer(sb), hip_rt.DeviceBuffer(rb + GUARD)
        sc, sd, rc_, rd = sh.args(rank)

        def prepare(seed):
            mine = sh.my_send(seed, rank)
            b.fill_byte(FILL)
            a.upload(mine)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            return np.concatenate([sh.my_expect(seed, rank), np.full(GUARD, FILL, np.uint8)])

        prepare(300)
        rcs = []
        issue = lambda: rcs.append(comm.all_to_all_v(a.ptr, sc, sd, b.ptr, rc_, rd, M.ncclFloat, st.handle))
        out = {"bad": []}
        if algo == M_RING:
            # the call is refused: begin and end the capture by hand, the empty graph is only destroyed
            L, g = hip_rt.lib(), ctypes.c_void_p()
            hip_rt.check(L.hipStreamBeginCapture(st.handle, 0), "hipStreamBeginCapture")
            try:
                issue()
            finally:
                hip_rt.check(L.hipStreamEndCapture(st.handle, ctypes.byref(g)), "hipStreamEndCapture")
            L.hipGraphDestroy(g.value)
        else:
            g = hip_rt.Graph(st, issue)
            for k in range(replays if rcs == [0] else 0):
                exp = prepare(301 + k)
                g.launch()
                st.sync()
                out["bad"].append(_differ(b.download(np.uint8, rb + GUARD), exp)[0])
            g.destroy()
        out.update(capture_rc=rcs, captured_algo=comm.info()["last_algo"])
        exp = prepare(400)
        out["eager_rc"] = comm.all_to_all_v(a.ptr, sc, sd, b.ptr, rc_, rd, M.ncclFloat, st.handle)
        st.sync()
        out["eager_algo"] = comm.info()["last_algo"]
        out["eager_bad"] = _differ(b.download(np.uint8, rb + GUARD), exp)[0]
        out.update(_info_fields(comm))
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def one_rank(port, env, out_q):
    """nranks == 1: a copy of block 0 between displacements, on both schedule settings; a count
    mismatch is ncclInvalidUsage and an all-zero call writes nothing."""
    try:
        hip_rt, M, comm, st = _open(0, 1, port, env, M_READ)
        c, sdis, rdis = 4099, 5, 11
        a, b = hip_rt.DeviceBuffer((c + sdis) * 2), hip_rt.DeviceBuffer((c + rdis) * 2 + GUARD)
        mine = np.frombuffer(np.random.default_rng(5).bytes((c + sdis) * 2), np.uint8)
        a.upload(mine)
        out = {"rcs": [], "bad": []}
        for algo, counts in ((M_READ, ([c], [c])), (M_RING, ([c], [c])), (M_READ, ([c], [c - 1])), (M_READ, ([0], [0]))):
            comm.set_algo(algo)
            b.fill_byte(FILL)
            hip_rt.sync()
            rc = comm.all_to_all_v(a.ptr, counts[0], [sdis], b.ptr, counts[1], [rdis], M.ncclBfloat16, st.handle)
            st.sync()
            exp = np.full((c + rdis) * 2 + GUARD, FILL, np.uint8)
            if rc == 0 and counts[0][0]:
                exp[rdis * 2:(rdis + c) * 2] = mine[sdis * 2:(sdis + c) * 2]
            out["rcs"].append(rc)
            out["bad"].append(_differ(b.download(np.uint8, exp.size), exp)[0])
        out["async"] = comm.async_error()
        a.free()
        b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((0, out))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))
