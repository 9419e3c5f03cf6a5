"""Rank processes for the mncclAllToAllvRows GPU tests (one process = one rank, as
tests/alltoallv_workers.py), and the reference both suites share: numpy fancy indexing, an index
outside [0, nrows) giving a row of zero bytes, every rank's matrix and index list derived from the
case's seed, compared as bytes.  A recv starts as FILL bytes: the row in front of its first block, the
gaps between its blocks and the 256 guard bytes behind it must come back unchanged.  The matrix sits
between MARGIN rows of MARK bytes: a bad index that escaped the check delivers MARK."""
import ctypes
import os
import traceback

import numpy as np

from alltoall_workers import FILL
from coll_workers import GUARD, _info_fields

NROWS, MARGIN, MARK = 48, 4, 0xEE
DTYPE_OF = {1: 10, 2: 9, 4: 7, 8: 8}  # ncclFloat8e4m3, ncclBfloat16, ncclFloat, ncclDouble: by element size


class Shape:
    """One call as every rank derives it from the case: C[r][q] rows of `rowcount` elements from r to q at
    stride rowcount + pad; idx "top2" (every index twice), "identity" or "oob" (top2 with -1, nrows and
    INT32_MAX among the valid ones); the ranges of rowidx overlap (sd), the recv blocks have gaps (rd)."""

    def __init__(self, case, n):
        self.n, self.esz, self.rowcount, self.mode = n, case["esz"], case["rowcount"], case.get("idx", "top2")
        self.C = np.array(case["C"], dtype=np.int64).reshape(n, n)
        self.stride, self.rb = self.rowcount + case.get("pad", 0), self.rowcount * self.esz
        self.sd = [[int(self.C[r, :q].sum()) // (1 + (self.mode != "identity")) for q in range(n)] for r in range(n)]
        self.rd = [[1 + int(self.C[:q, r].sum()) + q for q in range(n)] for r in range(n)]

    def matrix(self, seed, r):
        return np.random.default_rng([seed, r]).integers(0, 256, (NROWS, self.stride * self.esz), dtype=np.uint8)

    def rowidx(self, seed, r):
        used = max(self.sd[r][q] + int(self.C[r, q]) for q in range(self.n)) + 1
        if self.mode == "identity":
            return np.arange(used, dtype=np.int32)
        idx = np.repeat(np.random.default_rng([seed, r, 1]).integers(0, NROWS, used // 2 + 1), 2)[:used]
        if self.mode == "oob":
            idx[1::3] = np.resize((-1, NROWS, 2**31 - 1), idx[1::3].size)
        return idx.astype(np.int32)

    def recv_bytes(self, r):
        return (self.rd[r][-1] + int(self.C[-1, r]) + 1) * self.rb

    def expect(self, seed, q, mseed=None):  # mseed: the matrices' seed when only the indices were rewritten
        out = np.full(self.recv_bytes(q), FILL, np.uint8)
        for r in range(self.n):
            rows = self.rowidx(seed, r)[self.sd[r][q]:self.sd[r][q] + int(self.C[r, q])].astype(np.int64)
            ok = (rows >= 0) & (rows < NROWS)
            x = self.matrix(seed if mseed is None else mseed, r)
            got = np.where(ok[:, None], x[np.where(ok, rows, 0)][:, :self.rb], 0).astype(np.uint8)
            out[self.rd[q][r] * self.rb:(self.rd[q][r] + len(rows)) * self.rb] = got.reshape(-1)
        return out


def _case(comm, case, rank, n, st, barrier):
    """One case: C, esz, rowcount, pad, idx, algo, seed; send_off / recv_off (a misaligned base per
    rank); null_ranks (NULL buffers); bad (rank 1 passes rowcount + 1, or expects one row more from
    rank 0); vs_a2av (ncclAllToAllv on the same buffers must give the same recv); graph (captured, then
    replayed twice with rowidx rewritten in between)."""
    import hip_rt
    sh, seed = Shape(case, n), case.get("seed", 1)
    off, roff = case.get("send_off", [0] * n)[rank], case.get("recv_off", [0] * n)[rank]
    null = rank in case.get("null_ranks", ())
    row_b, mb, rb = sh.stride * sh.esz, NROWS * sh.stride * sh.esz, sh.recv_bytes(rank)
    sbuf, rbuf = hip_rt.DeviceBuffer(off + mb + 2 * MARGIN * row_b), hip_rt.DeviceBuffer(roff + rb + GUARD)
    ibuf, r2 = hip_rt.DeviceBuffer(4 * 512), hip_rt.DeviceBuffer(rb)
    sbuf.fill_byte(MARK)
    send = hip_rt.View(sbuf, off + MARGIN * row_b, mb)
    send.upload(sh.matrix(seed, rank))
    sc, sd, rc_, rd = [int(v) for v in sh.C[rank, :]], sh.sd[rank], [int(v) for v in sh.C[:, rank]], sh.rd[rank]
    rowcount = sh.rowcount + (1 if case.get("bad") == "rowcount" and rank == 1 else 0)
    if case.get("bad") == "count" and rank == 1:
        rc_ = [rc_[0] + 1] + rc_[1:]
    res = {"case": case, "bad": 0, "rcs": [], "algos": []}
    call = lambda: res["rcs"].append(comm.all_to_all_v_rows(
        None if null else send.ptr, NROWS, sh.stride, None if null else ibuf.ptr, sc, sd, None if null else rbuf.ptr + roff,
        rc_, rd, rowcount, DTYPE_OF[sh.esz], st.handle))

    def prepare(s):  # the index list of seed s in place, recv refilled; what recv and its guard must become
        ibuf.upload(sh.rowidx(s, rank))
        rbuf.fill_byte(FILL)  # (waits for the device)
        barrier.wait(120)
        return np.concatenate([sh.expect(s, rank, mseed=seed), np.full(GUARD, FILL, np.uint8)])

    def finish(exp):  # a refused call writes nothing
        st.sync()
        want = exp if res["rcs"] == [0] else np.full(rb + GUARD, FILL, np.uint8)
        res["bad"] += int((rbuf.download(np.uint8, rb + GUARD, roff) != want).sum())
        res["algos"].append(comm.info()["last_algo"])

    exp = prepare(seed)
    if case.get("graph") and case["algo"] == 0:  # refused: the empty graph is only destroyed, never instantiated
        L, g = hip_rt.lib(), ctypes.c_void_p()
        hip_rt.check(L.hipStreamBeginCapture(st.handle, 0), "hipStreamBeginCapture")
        call()
        hip_rt.check(L.hipStreamEndCapture(st.handle, ctypes.byref(g)), "hipStreamEndCapture")
        L.hipGraphDestroy(g.value)
        finish(exp)
    elif case.get("graph"):
        g = hip_rt.Graph(st, call)
        for s in (seed + 100, seed + 200) if res["rcs"] == [0] else ():
            exp = prepare(s)
            g.launch()
            finish(exp)
        g.destroy()
    else:
        call()
        finish(exp)
    if case.get("vs_a2av"):
        r2.fill_byte(FILL)
        e = lambda v: [x * sh.rowcount for x in v]
        assert comm.all_to_all_v(send.ptr, e(sc), e(sd), r2.ptr, e(rc_), e(rd), DTYPE_OF[sh.esz], st.handle) == 0
        st.sync()
        res["bad"] += int((r2.download(np.uint8, rb) != rbuf.download(np.uint8, rb, roff)).sum())
    res["bad"] += int((sbuf.download(np.uint8, off + MARGIN * row_b) != MARK).sum())  # the send side is only read
    res.update(_info_fields(comm))
    for b in (sbuf, rbuf, ibuf, r2):
        b.free()
    return res


def rows_rank(rank, n, port, cases, env, out_q, barrier=None):
    try:
        os.environ.update(env)
        os.environ["MINI_NCCL_PORT"] = str(port)
        import hip_rt
        import mini_nccl as M
        from gpu_workers import use_rank_device
        use_rank_device(rank)
        comm = M.Comm(n, rank, "127.0.0.1")
        st = hip_rt.Stream()
        results = []
        for case in cases:
            comm.set_algo(case["algo"])
            results.append(_case(comm, case, rank, n, st, barrier))
        st.destroy()
        out_q.put((rank, {"results": results, "destroy": comm.destroy()}))
    except Exception:
        out_q.put((rank, {"error": traceback.format_exc()}))
