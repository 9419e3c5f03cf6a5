"""Rank processes for the mncclAllToAllvCombine GPU tests (one process = one rank, as rows_workers.py),
and their reference: the rule of mini_nccl_ext.h restated in numpy -- np.float32 products and sums in
slot order, a slot outside every block skipped, one final rounding (astype for fp16, integer
round-to-nearest-even for bf16) -- compared bit for bit.  recv starts as FILL bytes: the elements
between rows and the guard bytes behind it must come back unchanged."""
import ctypes
import os
import traceback

import numpy as np

from alltoall_workers import FILL
from coll_workers import GUARD, _info_fields

NCCL = {"f32": 7, "f16": 6, "bf16": 9}
ESZ = {"f32": 4, "f16": 2, "bf16": 2}


def _bf16(y):  # float32 -> bf16 bits, to nearest even
    u = y.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


class Shape:
    """One call as every rank derives it: C[r][q] rows go from rank r's send back to rank q.  Both sides
    have gaps: sd[r][q] in r's dense send, rd[r][q] in r's virtual sequence.  nrows[r] output rows of
    `topk` slots each: valid positions mixed with -1, positions in a gap, beyond the last block and
    INT32_MAX; every 7th token has no valid slot at all."""

    def __init__(self, case, n):
        self.n, self.dt, self.rowcount, self.topk = n, case["dtype"], case["rowcount"], case["topk"]
        self.C = np.array(case["C"], dtype=np.int64).reshape(n, n)
        self.nrows = [case["nrows"][r % len(case["nrows"])] for r in range(n)]
        self.stride, self.esz, self.weighted = self.rowcount + case.get("pad", 0), ESZ[self.dt], case.get("weights", True)
        self.sd = [[1 + int(self.C[r, :q].sum()) + q for q in range(n)] for r in range(n)]
        self.rd = [[2 + int(self.C[:q, r].sum()) + 2 * q for q in range(n)] for r in range(n)]
        self.send_rows = [self.sd[r][-1] + int(self.C[r, -1]) + 1 for r in range(n)]

    def send(self, seed, r):  # float32 values exactly representable in the datatype
        x = np.random.default_rng([seed, r]).standard_normal((self.send_rows[r], self.rowcount)).astype(np.float32)
        return x.astype(np.float16).astype(np.float32) if self.dt == "f16" else \
            (x.view(np.uint32) & 0xFFFF0000).view(np.float32) if self.dt == "bf16" else x

    def bits(self, y):  # float32 -> the datatype's bytes, rounded once
        return (y.astype(np.float16) if self.dt == "f16" else _bf16(y) if self.dt == "bf16" else y).view(np.uint8)

    def slots(self, seed, r):
        rng, end = np.random.default_rng([seed, r, 1]), self.rd[r][-1] + int(self.C[-1, r])
        valid = np.concatenate([np.arange(self.rd[r][q], self.rd[r][q] + self.C[q, r]) for q in range(self.n)] + [[-1]])
        odd = np.array([-1, -7, end, end + 5, 2**31 - 1, self.rd[r][0] - 1, self.rd[r][-1] - 1])
        s = np.where(rng.random((self.nrows[r], self.topk)) < 0.75, rng.choice(valid, (self.nrows[r], self.topk)),
                     rng.choice(odd, (self.nrows[r], self.topk)))
        s[3::7] = rng.choice(odd, s[3::7].shape)
        return s.astype(np.int32), rng.standard_normal((self.nrows[r], self.topk)).astype(np.float32)

    def expect(self, seed, r, dseed=None):  # dseed: the data's seed when only slots and weights were rewritten
        if self.nrows[r] == 0:
            return np.zeros(0, np.uint8)
        s, w = self.slots(seed, r)
        y = np.zeros((self.nrows[r], self.rowcount), np.float32)
        xs = [self.send(seed if dseed is None else dseed, q) for q in range(self.n)]
        for k in range(self.topk):
            for q in range(self.n):
                j = s[:, k].astype(np.int64) - self.rd[r][q]
                ok = (j >= 0) & (j < self.C[q, r])
                x = xs[q][self.sd[q][r] + np.where(ok, j, 0)]
                wk = w[:, k, None] if self.weighted else np.float32(1)
                y = np.where(ok[:, None], y + (wk * x).astype(np.float32), y)
        out = np.full((self.nrows[r], self.stride * self.esz), FILL, np.uint8)
        out[:self.nrows[r], :self.rowcount * self.esz] = self.bits(y).reshape(self.nrows[r], -1)
        return out.reshape(-1)[:self.recv_bytes(r)]

    def recv_bytes(self, r):
        return ((self.nrows[r] - 1) * self.stride + self.rowcount) * self.esz if self.nrows[r] else 0


def _case(comm, case, rank, n, st, barrier):
    """One case: C, dtype, rowcount, pad, topk, weights, nrows, algo, seed; send_off / recv_off (a
    misaligned base per rank); over (rank 1's, or with over_all every rank's, arguments replaced: the
    refusals); graph (captured, then replayed twice with slotidx and weights rewritten in between);
    dispatch (mncclAllToAllvRows first: topk 1, NULL weights and the inverse index bring the tokens back)."""
    import hip_rt
    sh, seed = Shape(case, n), case.get("seed", 1)
    off, roff = case.get("send_off", [0] * n)[rank], case.get("recv_off", [0] * n)[rank]
    nr, rb = sh.nrows[rank], sh.recv_bytes(rank)
    sbuf, rbuf = hip_rt.DeviceBuffer(off + sh.send_rows[rank] * sh.rowcount * sh.esz + 16), hip_rt.DeviceBuffer(roff + rb + GUARD)
    ibuf, wbuf = hip_rt.DeviceBuffer(4 * nr * sh.topk + 16), hip_rt.DeviceBuffer(4 * nr * sh.topk + 16)
    a = dict(send=sbuf.ptr + off, sc=[int(v) for v in sh.C[rank, :]], sd=sh.sd[rank], recv=rbuf.ptr + roff, nrows=nr,
             stride=sh.stride, idx=ibuf.ptr, w=wbuf.ptr if sh.weighted else None, topk=sh.topk,
             rc=[int(v) for v in sh.C[:, rank]], rd=sh.rd[rank], rowcount=sh.rowcount)
    host = np.zeros(max(nr * sh.topk, 1), np.int32)  # pageable: refused as a list
    if rank == 1 or case.get("over_all"):
        a.update({k: {"HOST": host.ctypes.data, "W": wbuf.ptr}.get(v, v) if isinstance(v, str) else v
                  for k, v in case.get("over", {}).items()})
    res = {"case": case, "bad": 0, "rcs": [], "algos": []}
    import mini_nccl as M
    grouped = lambda f: (M.load().ncclGroupStart(), f(), M.load().ncclGroupEnd())[1] if case.get("group") else f()
    call = lambda: res["rcs"].append(grouped(lambda: comm.all_to_all_v_combine(
        a["send"], a["sc"], a["sd"], a["recv"], a["nrows"], a["stride"], a["idx"], a["w"], a["topk"], a["rc"], a["rd"],
        a["rowcount"], NCCL[sh.dt], st.handle)))

    def prepare(s):  # slots and weights of seed s in place, recv refilled; what recv and its guard must become
        slots, w = sh.slots(s, rank)
        ibuf.upload(slots)
        wbuf.upload(w)
        rbuf.fill_byte(FILL)  # (waits for the device)
        barrier.wait(120)
        return np.concatenate([sh.expect(s, rank, dseed=seed), np.full(GUARD, FILL, np.uint8)])

    def finish(exp):  # a refused call writes nothing
        st.sync()
        want = exp if res["rcs"][-1] == 0 else np.full(rb + GUARD, FILL, np.uint8)
        res["bad"] += int((rbuf.download(np.uint8, rb + GUARD, roff) != want).sum())
        res["algos"].append(comm.info()["last_algo"])

    sbuf.upload(sh.bits(sh.send(seed, rank)), off)
    exp = prepare(seed)
    bufs = [sbuf, rbuf, ibuf, wbuf]
    if case.get("dispatch"):  # tokens out by rows, back by the combine: C transposed, every token routed once
        sc, rc_ = a["rc"], a["sc"]
        sd, rd = np.concatenate([[0], np.cumsum(sc)[:-1]]).tolist(), np.concatenate([[0], np.cumsum(rc_)[:-1]]).tolist()
        ntok, row_b = sum(sc), sh.rowcount * sh.esz
        perm = np.random.default_rng([seed, rank, 2]).permutation(ntok).astype(np.int32)
        tok = np.random.default_rng([seed, rank, 3]).integers(0, 256, (ntok, row_b), dtype=np.uint8) & 0x7B  # (no NaN, no -0)
        tbuf, ebuf, ybuf, pbuf = [hip_rt.DeviceBuffer(max(x, 1) * row_b + 16) for x in (ntok, sum(rc_), ntok, ntok)]
        bufs += [tbuf, ebuf, ybuf, pbuf]
        tbuf.upload(tok), pbuf.upload(perm), ibuf.upload(np.argsort(perm).astype(np.int32))
        barrier.wait(120)
        assert comm.all_to_all_v_rows(tbuf.ptr, ntok, sh.rowcount, pbuf.ptr, sc, sd, ebuf.ptr, rc_, rd, sh.rowcount, NCCL[sh.dt],
                                      st.handle) == 0
        res["rcs"].append(comm.all_to_all_v_combine(ebuf.ptr, rc_, rd, ybuf.ptr, ntok, sh.rowcount, ibuf.ptr, None, 1, sc, sd,
                                                    sh.rowcount, NCCL[sh.dt], st.handle))
        st.sync()
        res["bad"] += int((ybuf.download(np.uint8, ntok * row_b) != tok.reshape(-1)).sum())
        res["algos"].append(comm.info()["last_algo"])
    elif case.get("graph") and case["algo"] == 0:  # refused: the empty graph is only destroyed, never instantiated
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
    res.update(_info_fields(comm))
    for b in bufs:
        b.free()
    return res


def combine_rank(rank, n, port, cases, env, out_q, barrier=None):
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
