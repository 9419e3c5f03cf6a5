"""Rank processes for the mncclAllToAllvRowsMxfp4 GPU tests: rowsmx_workers' case with records of P4 bytes, mx4_ref and the MXFP4 entry."""
import numpy as np

import mx4_ref
import rowsmx_workers as MW

_mx_case, _mx_rank = MW._case, MW.mx_rank  # (taken at import: the GPU tests put mx4_rank in MW.mx_rank's place)


class Shape(MW.Shape):
    def __init__(self, case, n):
        super().__init__(case, n)
        self.mixed = case.get("bad") == "mxfp8"  # recv then holds what rank 1's MXFP8 call describes, or its local checks refuse first
        self.rb = self.rowcount // (1 if self.mixed else 2) + self.rowcount // 32

    def expect(self, seed, q, mseed=None):  # (the mixed call is refused everywhere: recv stays FILL)
        return np.full(self.recv_bytes(q), MW.FILL, np.uint8) if self.mixed else super().expect(seed, q, mseed)


def _case(comm, case, rank, n, st, barrier):
    """rowsmx_workers._case with the MXFP4 entry under the name it calls; bad "mxfp8": rank 1 keeps the MXFP8 entry."""
    entry = "all_to_all_v_rows_mxfp8" if case.get("bad") == "mxfp8" and rank == 1 else "all_to_all_v_rows_mxfp4"
    comm.all_to_all_v_rows_mxfp8 = getattr(type(comm), entry).__get__(comm)
    return _mx_case(comm, case, rank, n, st, barrier)


def mx4_rank(*args, **kw):
    MW._case, MW.Shape, MW.mx_ref = _case, Shape, mx4_ref  # (in the rank's own process) this file's case, shape and reference
    return _mx_rank(*args, **kw)
