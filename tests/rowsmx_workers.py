"""Rank processes for the mncclAllToAllvRowsMxfp8 GPU tests: rows_workers' layout (FILL around the recv
blocks, MARK rows around the matrix, the same counts, displacements and index lists) with records of
P = rowcount + rowcount // 32 bytes on the receive side and mx_ref.quantise for the expected bytes."""
import ctypes

import numpy as np

import mx_ref
import rows_workers as RW
from alltoall_workers import FILL
from coll_workers import GUARD, _info_fields

NCCL_OF = {"bf16": 9, "f16": 6, "f32": 7}


class Shape(RW.Shape):
    """rows_workers.Shape, 2-byte elements, recv rows are records; case["sweep"]: the first rows are mx_ref.sweep."""

    def __init__(self, case, n):
        super().__init__(dict(case, esz=2), n)
        self.f16, self.sweep = case.get("dtype", "bf16") == "f16", case.get("sweep", False)
        self.rb = self.rowcount + self.rowcount // 32

    def matrix(self, seed, r):
        x = super().matrix(seed, r)
        if self.sweep:
            s = mx_ref.sweep(self.f16).reshape(-1, self.rowcount)
            x.view(np.uint16)[:s.shape[0], :self.rowcount] = s
        return x

    def expect(self, seed, q, mseed=None):
        out = np.full(self.recv_bytes(q), FILL, np.uint8)
        for r in range(self.n):
            rows = self.rowidx(seed, r)[self.sd[r][q]:self.sd[r][q] + int(self.C[r, q])].astype(np.int64)
            if rows.size == 0:
                continue
            ok = (rows >= 0) & (rows < RW.NROWS)
            x = self.matrix(seed if mseed is None else mseed, r).view(np.uint16)[:, :self.rowcount]
            got = mx_ref.quantise(np.where(ok[:, None], x[np.where(ok, rows, 0)], 0), self.f16)
            out[self.rd[q][r] * self.rb:(self.rd[q][r] + len(rows)) * self.rb] = got.reshape(-1)
        return out


def _case(comm, case, rank, n, st, barrier):
    """rows_workers._case's keys, and dtype, sweep, recv_off (a misaligned recv on every rank)."""
    import hip_rt
    sh, seed, roff = Shape(case, n), case.get("seed", 1), case.get("recv_off", 0)
    null = rank in case.get("null_ranks", ())
    row_b, rb = sh.stride * 2, sh.recv_bytes(rank)
    sbuf, rbuf, ibuf = (hip_rt.DeviceBuffer(b) for b in ((RW.NROWS + 2 * RW.MARGIN) * row_b, roff + rb + GUARD, 4 * 512))
    sbuf.fill_byte(RW.MARK)
    send = hip_rt.View(sbuf, RW.MARGIN * row_b, RW.NROWS * row_b)
    send.upload(sh.matrix(seed, rank))
    sc, sd, rc_, rd = [int(v) for v in sh.C[rank, :]], sh.sd[rank], [int(v) for v in sh.C[:, rank]], sh.rd[rank]
    rowcount = sh.rowcount + (128 if case.get("bad") == "rowcount" and rank == 1 else 0)
    if case.get("bad") == "count" and rank == 1:
        rc_ = [rc_[0] + 1] + rc_[1:]
    res = {"case": case, "bad": 0, "rcs": [], "algos": []}
    call = lambda: res["rcs"].append(comm.all_to_all_v_rows_mxfp8(
        None if null else send.ptr, RW.NROWS, sh.stride, None if null else ibuf.ptr, sc, sd, None if null else rbuf.ptr + roff,
        rc_, rd, rowcount, NCCL_OF[case.get("dtype", "bf16")], st.handle))

    def prepare(s):
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
    res["bad"] += int((sbuf.download(np.uint8, RW.MARGIN * row_b) != RW.MARK).sum())  # the send side is only read
    res["bad"] += int((send.download(np.uint8, RW.NROWS * row_b) != sh.matrix(seed, rank).reshape(-1)).sum())
    res.update(_info_fields(comm))
    for b in (sbuf, rbuf, ibuf):
        b.free()
    return res


def mx_rank(*args, **kw):
    RW._case = _case  # (in the rank's own process) rows_workers' rank loop around this file's case
    return RW.rows_rank(*args, **kw)
