"""combine_workers' case and shape with MXFP8 records on the send side, the entry under the name the case calls; NaN as NaN."""
import numpy as np

import combine_workers as CW
import mx_ref
import mxc_ref

_cw_case, _cw_rank = CW._case, CW.combine_rank


class Shape(CW.Shape):
    """send() is the DECODED block, so combine_workers.Shape.expect folds it unchanged; bits() of exactly that array is the
    records' bytes (the case's upload), of anything else the rounding.  sweep: every e4m3 code at mxc_ref.SCALES[i % 8]."""

    def __init__(self, case, n):
        super().__init__(case, n)
        self.case, self.sent, self.P = case, None, self.rowcount + self.rowcount // 32

    def rows(self, seed, r):
        rng, shape = np.random.default_rng([seed, r]), (self.send_rows[r], self.rowcount // 32)
        x = rng.standard_normal(shape + (32,)) * 2.0 ** rng.integers(-30, 30, shape + (1,))
        return (x.astype(np.float32).reshape(shape[0], -1).view(np.uint32) >> 16).astype(np.uint16)

    def send(self, seed, r):
        self.recs = mx_ref.quantise(self.rows(seed, r), False)
        if self.case.get("sweep"):
            self.recs[:, :self.rowcount] = np.tile(np.arange(256, dtype=np.uint8), self.rowcount // 256)
            self.recs[:, self.rowcount:] = np.array(mxc_ref.SCALES, np.uint8)[np.arange(len(self.recs)) % 8, None]
        self.sent = mxc_ref.decode(self.recs, self.rowcount)
        return self.sent

    def bits(self, y):
        return self.recs.reshape(-1) if y is self.sent else mxc_ref.canon(np.ravel(super().bits(y)), self.dt)

    def slots(self, seed, r):
        s, w = super().slots(seed, r)
        return s, np.full_like(w, self.case["w_const"]) if "w_const" in self.case else w


def _dispatch_into(comm, sh, seed, rank, st, send, sc, sd):
    """The send buffer cleared and refilled by mncclAllToAllvRowsMxfp8 from the bf16 rows its records were made of."""
    import hip_rt
    src = [sh.rows(seed, r)[sh.sd[r][rank]:sh.sd[r][rank] + int(sh.C[r, rank])] for r in range(sh.n)]
    tok, out = np.concatenate(src), [len(x) for x in src]
    tbuf, pbuf = hip_rt.DeviceBuffer(tok.nbytes + 16), hip_rt.DeviceBuffer(4 * len(tok) + 16)
    tbuf.upload(tok), pbuf.upload(np.arange(len(tok), dtype=np.int32))
    hip_rt.check(hip_rt.lib().hipMemset(send, 0, sh.send_rows[rank] * sh.P), "hipMemset")
    hip_rt.sync()
    rc = comm.all_to_all_v_rows_mxfp8(tbuf.ptr, len(tok), sh.rowcount, pbuf.ptr, out, np.cumsum([0] + out[:-1]).tolist(),
                                      send, sc, sd, sh.rowcount, CW.NCCL["bf16"], st.handle)
    st.sync()
    tbuf.free(), pbuf.free()
    assert rc == 0, rc


def _case(comm, case, rank, n, st, barrier):
    """mx_over (rank 1's, with over_all everyone's): plain (the plain combine instead), dt (a type code), send_add / recv_add."""
    import hip_rt
    o = case.get("mx_over", {}) if rank == 1 or case.get("over_all") else {}
    entry = type(comm).all_to_all_v_combine if o.get("plain") else type(comm).all_to_all_v_combine_mxfp8

    def call(send, sc, sd, recv, *a):
        if case.get("mx_dispatch"):
            _dispatch_into(comm, Shape(case, n), case["seed"], rank, st, send, sc, sd)
        return entry(comm, send and send + o.get("send_add", 0), sc, sd, recv and recv + o.get("recv_add", 0), *a[:-2],
                     o.get("dt", a[-2]), a[-1])
    download, comm.all_to_all_v_combine = hip_rt.DeviceBuffer.download, call
    hip_rt.DeviceBuffer.download = lambda self, t, count, off=0: mxc_ref.canon(download(self, t, count, off), case["dtype"])
    try:
        return _cw_case(comm, case, rank, n, st, barrier)
    finally:
        hip_rt.DeviceBuffer.download = download


def combinemx_rank(*args, **kw):
    CW._case, CW.Shape = _case, Shape  # (in the rank's own process) combine_workers' rank loop around this file's case and shape
    return _cw_rank(*args, **kw)
