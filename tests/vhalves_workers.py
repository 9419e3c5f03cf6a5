"""Rank processes for the mncclAllGatherv / mncclReduceScatterv GPU tests (one process = one rank;
placement, spawning and the consumer kernels are tests/gpu_workers.py's).

A call's shape is sim_vhalves_api.Shape: n counts, n displacements and the array-side buffer's length,
the same on every rank.  Every rank derives every rank's seeded inputs, so it computes what it must
receive without the others' buffers:
  gather -- rank q sends counts[q] elements of seeded random BYTES; every recv is FILL bytes with rank
            q's block at displs[q], compared as bytes (gaps and the guard behind recv included);
  fold   -- rank q's send holds `length` elements (make_inputs / fp8_ref.inputs); rank r's recv is the
            reference fold on block c laid into chunk c (oracle_api.ring_fold; premul_ref.prescale in
            front of it for a pre-multiplied sum; fp8_ref.ring_fold for the fp8 types), bit for bit.
"""
import ctypes
import os
import threading
import time
import traceback

import numpy as np

from coll_workers import GUARD, _info_fields, per_rank
from gpu_workers import compare, make_inputs, testkern, use_rank_device
from sim_vhalves_api import FILL, Shape

M_RING, M_READ = 0, 2
FP8 = ("e4m3", "e5m2")


def dtype_info(dtype):
    """(ncclDataType_t, numpy storage type)"""
    import fp8_ref as F
    import oracle_api as O
    return (F.code(dtype), np.uint8) if dtype in FP8 else O.DTYPES[dtype]


def shape_of(case, n):
    sh = Shape(case["counts"], case.get("mode", "contig"))
    assert sh.n == n
    if "displs" in case:
        sh.displs = [int(d) for d in case["displs"]]
        sh.length = max(d + c for d, c in zip(sh.displs, sh.counts)) + case.get("slack", 0)
    return sh


def fold_inputs(n, sh, dtype, seed, case):
    import fp8_ref as F
    if dtype in FP8:
        return F.inputs(n, sh.length, dtype, seed, case.get("kind", "plain"))
    return make_inputs(n, sh.length, dtype, seed, case.get("special", False))


def fold_expect(sh, xs, dtype, op, s=None):
    """Every rank's recv (a list): the reference fold on block c laid into chunk c of n x max(counts)."""
    import fp8_ref as F
    import oracle_api as O
    import premul_ref as P
    if sh.M == 0:
        return [xs[0][:0] for _ in range(sh.n)]
    laid = sh.laid_out(xs)
    if dtype in FP8:
        full = F.ring_fold(laid, dtype, op, s)
    elif op == "premul":
        full = O.ring_fold([P.prescale(x, s, dtype) for x in laid], dtype, "sum")
    else:
        full = O.ring_fold(laid, dtype, op)
    return [full[r * sh.M:r * sh.M + sh.counts[r]] for r in range(sh.n)]


def differ(got, exp, dtype, op):
    import fp8_ref as F
    if dtype in FP8:
        return F.mismatches(got, exp, dtype)
    return compare(got, exp, dtype, op in ("sum", "prod", "premul"))


def make_op(comm, M, dtype, op, s):
    """(op argument, handle to destroy or None)"""
    import fp8_ref as F
    import premul_ref as P
    code = dtype_info(dtype)[0]
    if op != "premul":
        return F.OP_CODE[op], None
    h = comm.redop_premul_sum(int(s) if dtype in FP8 else P.scalar_arg(s, dtype), code)
    return h, h


def gather_blocks(sh, seed, esz):
    return sh.blocks(seed, esz)


def run_case(comm, case, rank, n, stream, barrier, hip_rt, M):
    """One case on an open communicator.  coll "agv" / "rsv"; dtype; op ("sum" / "prod" / "max" / "min" /
    "premul" with s); counts, mode or displs; algo; inplace; mem (the array side) / one_mem (the one
    block), each a value or a per-rank list; null_one (ranks whose block is empty pass NULL for the one
    block), null_all (every pointer NULL: an all-zero call); seed; calls (new data every call); special."""
    coll, dtype, op, seed = case["coll"], case["dtype"], case.get("op", "sum"), case.get("seed", 1)
    code, npd = dtype_info(dtype)
    esz = np.dtype(npd).itemsize
    sh = shape_of(case, n)
    c, d = sh.counts[rank], sh.displs[rank]
    inplace = case.get("inplace", False)
    gather = coll == "agv"
    mem_a = per_rank(case.get("mem", "device"), rank)
    mem_o = per_rank(case.get("one_mem", mem_a), rank)
    ab = sh.length * esz
    abuf = hip_rt.buffer(mem_a, ab + GUARD)
    arr, aguard = hip_rt.View(abuf, 0, ab), hip_rt.View(abuf, ab, GUARD)
    if inplace:
        obuf, one, oguard = None, hip_rt.View(abuf, d * esz, max(c, 1) * esz), None
    else:
        obuf = hip_rt.buffer(mem_o, max(c, 1) * esz + GUARD)
        one, oguard = hip_rt.View(obuf, 0, max(c, 1) * esz), hip_rt.View(obuf, max(c, 1) * esz, GUARD)
    null_one = case.get("null_all") or (c == 0 and case.get("null_one"))
    a_ptr = None if case.get("null_all") else arr.ptr
    o_ptr = None if null_one else one.ptr
    opc, handle = (0, None) if gather else make_op(comm, M, dtype, op, case.get("s"))
    bad, first, detail, rc, algos = 0, -1, "", 0, []
    t0 = time.time()
    for k in range(case.get("calls", 1)):
        sd = seed + 1000 * k
        abuf.fill_byte(FILL)
        if obuf is not None:
            obuf.fill_byte(FILL)
        if gather:
            blocks = gather_blocks(sh, sd, esz)
            exp = sh.gather_expect(blocks, esz)
            if c:
                one.upload(blocks[rank])
        else:
            xs = fold_inputs(n, sh, dtype, sd, case)
            exp = fold_expect(sh, xs, dtype, op, case.get("s"))[rank]
            arr.upload(xs[rank])
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        if gather:
            rc = comm.all_gather_v(o_ptr, c, a_ptr, sh.counts, sh.displs, code, stream.handle)
        else:
            rc = comm.reduce_scatter_v(a_ptr, sh.counts, sh.displs, o_ptr, c, code, opc, stream.handle)
        if rc != 0:
            bad = -1
            break
        stream.sync()
        algos.append(comm.info()["last_algo"])
        b = 0
        if gather:
            got = arr.download(np.uint8, ab)
            b, f = compare(got, exp, "u8", False)
            if b and not bad:
                first, detail = f, f"call {k}: byte {f} of recv got {got[f]} expected {exp[f]}"
            if not inplace and c:
                b += compare(one.download(np.uint8, c * esz), blocks[rank], "u8", False)[0]  # the send is only read
        else:
            if c:
                got = one.download(npd, c)
                b, f = differ(got, exp, dtype, op)
                if b and not bad:
                    first, detail = f, f"call {k}: element {f} of recv got {got[f]!r} expected {exp[f]!r}"
            # the send is only read -- in place: everything outside the own block
            after, was = arr.download(np.uint8, ab), np.ascontiguousarray(xs[rank]).view(np.uint8)
            keep = np.ones(ab, bool)
            if inplace:
                keep[d * esz:(d + c) * esz] = False
            b += int((after[keep] != was[keep]).sum())
        b += int((aguard.download(np.uint8, GUARD) != FILL).sum())
        if oguard is not None:
            b += int((oguard.download(np.uint8, GUARD) != FILL).sum())  # nothing written past the one block
        bad += b
    drc = comm.redop_destroy(handle) if handle is not None else 0
    res = {"case": case, "rc": rc, "bad": bad, "first": first, "detail": detail, "algos": algos, "destroy_op": drc,
           "secs": time.time() - t0}
    res.update(_info_fields(comm))
    res["window_calls"] = comm.info()["window_calls"]
    abuf.free()
    if obuf is not None:
        obuf.free()
    return res


def _open(rank, n, port, env, algo=None):
    os.environ.update(env)
    os.environ["MINI_NCCL_PORT"] = str(port)
    import hip_rt
    import mini_nccl as M
    use_rank_device(rank)
    comm = M.Comm(n, rank, "127.0.0.1")
    if algo is not None:
        comm.set_algo(algo)
    return hip_rt, M, comm, hip_rt.Stream()


def vh_rank(rank, n, port, cases, env, out_q, barrier=None):
    """Run `cases` (run_case) on one communicator, every call checked."""
    try:
        hip_rt, M, comm, stream = _open(rank, n, port, env)
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            results.append(run_case(comm, case, rank, n, stream, barrier, hip_rt, M))
        stream.destroy()
        info = comm.info()
        out_q.put((rank, {"results": results, "destroy": comm.destroy(), "info": info}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def split_rank(rank, n, port, cases, env, out_q, barrier=None):
    """The cases on a child of ncclCommSplit: ranks of the same parity form a child, ordered by rank.
    The children run at the same time; the parent's barrier cannot pace a child's calls, so none is used."""
    try:
        hip_rt, M, comm, stream = _open(rank, n, port, env)
        child = comm.split(rank % 2, rank)
        cn, cr = child.count(), child.rank()
        results = []
        for case in cases:
            child.set_algo(case["algo"])
            results.append(run_case(child, dict(case, counts=case["counts"][:cn]), cr, cn, stream, None, hip_rt, M))
        stream.destroy()
        out_q.put((rank, {"results": results, "child": (cn, cr), "destroy": (child.destroy(), comm.destroy())}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def threads_proc(n, port, cases, env, out_q):
    """Ranks as threads of one process, every rank a communicator of its own on the current device."""
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        use_rank_device(0)
        bar = threading.Barrier(n, timeout=120)
        out = [None] * n

        class Bar:
            def wait(self, _t):
                bar.wait()

        def main(r):
            try:
                use_rank_device(0)
                comm = M.Comm(n, r, "127.0.0.1")
                st = hip_rt.Stream()
                res = []
                for case in cases:
                    comm.set_algo(case["algo"])
                    res.append(run_case(comm, case, r, n, st, Bar(), hip_rt, M))
                bar.wait()
                st.destroy()
                out[r] = {"results": res, "destroy": comm.destroy()}
            except Exception:
                bar.abort()
                out[r] = {"error": traceback.format_exc()}

        ts = [threading.Thread(target=main, args=(r,)) for r in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(200)
        out_q.put((0, {"ranks": out}))
    except Exception:
        out_q.put((0, {"error": traceback.format_exc()}))


def pair_rank(rank, n, port, env, algo, dtype, counts, mode, rounds, out_q, barrier=None):
    """mncclReduceScatterv in place, then mncclAllGatherv in place with the same arrays on the same
    buffer: every block of the buffer is then its fold on every rank, the gaps what they were.  With
    uniform contiguous counts also: ncclReduceScatter / ncclAllGather / ncclAllReduce from the same
    inputs give the same bits (out of place, into buffers of their own)."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, algo)
        code, npd = dtype_info(dtype)
        esz = np.dtype(npd).itemsize
        sh = Shape(counts, mode)
        uniform = mode == "contig" and len(set(sh.counts)) == 1
        c, d, ab = sh.counts[rank], sh.displs[rank], sh.length * esz
        buf, src = hip_rt.DeviceBuffer(ab + GUARD), hip_rt.DeviceBuffer(ab)
        u_rs, u_ag, u_ar = (hip_rt.DeviceBuffer(ab) for _ in range(3))
        out = {"rcs": [], "bad": [], "bad_mid": [], "bad_uniform": [], "algos": []}
        for k in range(rounds):
            xs = fold_inputs(n, sh, dtype, 8000 + 13 * k, {})
            blocks = fold_expect(sh, xs, dtype, "sum")
            buf.fill_byte(FILL)
            buf.upload(xs[rank])
            src.upload(xs[rank])
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            rcs = [comm.reduce_scatter_v(buf.ptr, sh.counts, sh.displs, buf.ptr + d * esz, c, code, M.ncclSum, st.handle)]
            a1 = comm.info()["last_algo"]
            st.sync()
            mid = buf.download(npd, sh.length)
            rcs.append(comm.all_gather_v(buf.ptr + d * esz, c, buf.ptr, sh.counts, sh.displs, code, st.handle))
            st.sync()
            out["algos"].append((a1, comm.info()["last_algo"]))
            got = buf.download(npd, sh.length)
            exp_mid, exp = xs[rank].copy(), xs[rank].copy()
            exp_mid[d:d + c] = blocks[rank]
            for q in range(n):
                exp[sh.displs[q]:sh.displs[q] + sh.counts[q]] = blocks[q]
            out["bad_mid"].append(differ(mid, exp_mid, dtype, "sum")[0])
            out["bad"].append(differ(got, exp, dtype, "sum")[0] + int((buf.download(np.uint8, GUARD, ab) != FILL).sum()))
            if uniform:
                cnt = sh.counts[0]
                rcs.append(comm.reduce_scatter(src.ptr, u_rs.ptr, cnt, code, M.ncclSum, st.handle))
                rcs.append(comm.all_gather(u_rs.ptr, u_ag.ptr, cnt, code, st.handle))
                rcs.append(comm.all_reduce(src.ptr, u_ar.ptr, n * cnt, code, M.ncclSum, st.handle))
                st.sync()
                b = compare(u_rs.download(npd, cnt), mid[d:d + c], dtype, False)[0]       # the fold's bits
                b += compare(u_ag.download(npd, n * cnt), got, dtype, False)[0]           # the gather's
                b += compare(u_ar.download(npd, n * cnt), got, dtype, False)[0]           # the composition
                out["bad_uniform"].append(b)
            out["rcs"].append(rcs)
        out.update(_info_fields(comm))
        for b in (buf, src, u_rs, u_ag, u_ar):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def consumer_rank(rank, n, port, env, counts, rounds, out_q, barrier=None):
    """alltoallv_workers.consumer_rank's shape for vhalf_push's pushes: recv is first read by an
    ordinary kernel on the call's stream (its lines sit in this GPU's L2), then the call -- the peers
    push their blocks into this recv -- and an ordinary kernel copies recv with plain loads right
    behind the call on the same stream (MINI_NCCL_BLOCKING=0: no host wait in between)."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, M_READ)
        K = testkern()
        sh = Shape(counts, "contig")
        c, rb = sh.counts[rank], sh.length * 4
        send, recv, seen, word = (hip_rt.DeviceBuffer(x) for x in (max(c, 1) * 4, rb, rb, 256))
        recv.fill_byte(FILL)
        bad, rcs, algos = [], [], []
        for k in range(rounds):
            blocks = sh.blocks(6000 + k, 4)
            exp = sh.gather_expect(blocks, 4)
            send.upload(blocks[rank])
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            hip_rt.check(K.mnccl_test_touch(ctypes.c_void_p(recv.ptr), rb, ctypes.c_void_p(word.ptr),
                                            ctypes.c_void_p(st.handle)), "touch")
            rc = comm.all_gather_v(send.ptr, c, recv.ptr, sh.counts, sh.displs, M.ncclFloat, st.handle)
            hip_rt.check(K.mnccl_test_copy(ctypes.c_void_p(seen.ptr), ctypes.c_void_p(recv.ptr), rb,
                                           ctypes.c_void_p(st.handle)), "copy")
            st.sync()
            rcs.append(rc)
            algos.append(comm.info()["last_algo"])
            bad.append(compare(seen.download(np.uint8, rb), exp, "u8", False)[0])
        out = {"rcs": rcs, "bad": bad, "algos": algos}
        out.update(_info_fields(comm))
        for b in (send, recv, seen, word):
            b.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def refused_rank(rank, n, port, env, scenario, out_q, barrier=None):
    """The calls the library must refuse with a live communicator (n = 2, device buffers, read):
      local    -- check 4's cases: the scalar count off by one, a NULL buffer with a count, an
                  overflowing displacement, two blocks overlapping (both calls), the one-block buffer
                  laid over a block: ncclInvalidArgument each;
      entry    -- rank 1 passes one displacement one element further: ncclInvalidUsage on both ranks;
      count    -- rank 1 passes another count for rank 0's block: ncclInvalidUsage on both ranks;
      kinds    -- rank 0 calls mncclAllGatherv where rank 1 calls mncclReduceScatterv: ncclInvalidUsage;
      uniform  -- rank 0 calls mncclReduceScatterv where rank 1 calls ncclReduceScatter: ncclInvalidUsage;
      op       -- the ranks pass different built-in ops: ncclInvalidUsage.
    Nothing is written, mncclCommGetAsyncError is 0, and the next valid calls of both kinds are exact."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, M_READ)
        sh = Shape([4099, 1003], "gaps")
        c, d, ab = sh.counts[rank], sh.displs[rank], sh.length * 4
        a, o = hip_rt.DeviceBuffer(ab + GUARD), hip_rt.DeviceBuffer(c * 4 + GUARD)
        xs = fold_inputs(n, sh, "f32", 70, {})
        a.upload(xs[rank])
        o.fill_byte(FILL)
        hip_rt.sync()
        if barrier is not None:
            barrier.wait(120)
        F, S, h, top = M.ncclFloat, M.ncclSum, st.handle, (1 << 64) - 1
        rsv = lambda cs=sh.counts, ds=sh.displs, s=a.ptr, r=o.ptr, rc=c, op=S: comm.reduce_scatter_v(s, cs, ds, r, rc, F, op, h)
        agv = lambda cs=sh.counts, ds=sh.displs, s=o.ptr, r=a.ptr, sc=c: comm.all_gather_v(s, sc, r, cs, ds, F, h)
        if scenario == "local":
            over = [sh.displs[0], sh.displs[0] + 1]  # block 1 inside block 0
            rcs = [rsv(rc=c + 1), agv(sc=c - 1), rsv(r=None), agv(s=None), rsv(s=None), agv(r=None),
                   rsv(ds=[top, top]), agv(ds=[top - 4, top - 4]), rsv(ds=over), agv(ds=over),
                   rsv(r=a.ptr + 4 * d + 4), agv(s=a.ptr + 4 * sh.displs[1 - rank])]
        elif scenario == "entry":
            rcs = [rsv(ds=[sh.displs[0], sh.displs[1] + rank]), agv(ds=[sh.displs[0] + rank, sh.displs[1]])]
        elif scenario == "count":
            other = [sh.counts[0] - 1, sh.counts[1]] if rank == 1 else sh.counts
            rcs = [rsv(cs=other), agv(cs=other)]
        elif scenario == "kinds":
            rcs = [agv() if rank == 0 else rsv()]
        elif scenario == "uniform":
            rcs = [rsv() if rank == 0 else comm.reduce_scatter(a.ptr, o.ptr, 3, F, S, h)]
        else:
            rcs = [rsv(op=S if rank == 0 else M.ncclMax)]
        st.sync()
        out = {"rcs": rcs, "async_after": comm.async_error()}
        out["touched"] = int((o.download(np.uint8, c * 4 + GUARD) != FILL).sum())  # nothing was launched
        out["touched"] += compare(a.download(np.float32, sh.length), xs[rank], "f32", False)[0]
        out["next_rc"], out["next_bad"] = [], 0
        exp = fold_expect(sh, xs, "f32", "sum")[rank]
        rc = rsv()
        st.sync()
        out["next_rc"].append(rc)
        out["next_bad"] += compare(o.download(np.float32, c), exp, "f32", True)[0] if rc == 0 else 1
        blocks = sh.blocks(71, 4)
        o.upload(blocks[rank])
        a.fill_byte(FILL)
        hip_rt.sync()
        rc = agv()
        st.sync()
        out["next_rc"].append(rc)
        out["next_bad"] += compare(a.download(np.uint8, ab + GUARD), np.concatenate([sh.gather_expect(blocks, 4),
                                   np.full(GUARD, FILL, np.uint8)]), "u8", False)[0] if rc == 0 else 1
        out.update(_info_fields(comm))
        a.free()
        o.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))


def graph_rank(rank, n, port, env, algo, coll, counts, replays, out_q, barrier=None):
    """alltoallv_workers.graph_rank's pattern: ONE call captured into a HIP graph, replayed with new
    seeded inputs before every replay, then one eager call.  Under a forced ring the captured call is
    refused on every rank (the padded fallback's stage cannot be allocated inside a capture): the graph
    is empty, and the eager call still runs."""
    try:
        hip_rt, M, comm, st = _open(rank, n, port, env, algo)
        sh = Shape(counts, "gaps")
        c, ab = sh.counts[rank], sh.length * 4
        gather = coll == "agv"
        a, o = hip_rt.DeviceBuffer(ab + GUARD), hip_rt.DeviceBuffer(max(c, 1) * 4 + GUARD)

        def prepare(seed):
            """uploads the call's inputs; returns (buffer to check, expected bytes with the guard)"""
            a.fill_byte(FILL)
            o.fill_byte(FILL)
            if gather:
                blocks = sh.blocks(seed, 4)
                o.upload(blocks[rank])
                exp = sh.gather_expect(blocks, 4)
            else:
                xs = fold_inputs(n, sh, "f32", seed, {})
                a.upload(xs[rank])
                exp = np.ascontiguousarray(fold_expect(sh, xs, "f32", "sum")[rank]).view(np.uint8)
            hip_rt.sync()
            if barrier is not None:
                barrier.wait(120)
            return np.concatenate([exp, np.full(GUARD, FILL, np.uint8)])

        def bad(exp):
            got = (a if gather else o).download(np.uint8, exp.size)
            return compare(got, exp, "u8", False)[0]

        def call():
            if gather:
                return comm.all_gather_v(o.ptr, c, a.ptr, sh.counts, sh.displs, M.ncclFloat, st.handle)
            return comm.reduce_scatter_v(a.ptr, sh.counts, sh.displs, o.ptr, c, M.ncclFloat, M.ncclSum, st.handle)

        prepare(300)
        rcs = []
        issue = lambda: rcs.append(call())
        out = {"bad": []}
        if algo == M_RING:
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
                out["bad"].append(bad(exp))
            g.destroy()
        out.update(capture_rc=rcs, captured_algo=comm.info()["last_algo"])
        exp = prepare(400)
        out["eager_rc"] = call()
        st.sync()
        out["eager_algo"] = comm.info()["last_algo"]
        out["eager_bad"] = bad(exp)
        out.update(_info_fields(comm))
        a.free()
        o.free()
        st.destroy()
        out["destroy"] = comm.destroy()
        out_q.put((rank, out))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
