"""Rank processes for the mncclAllToAllvRowsFp8Block128 GPU tests: rowsmx_workers' case and shape (its records have this call's size) with fp8b_ref and the new entry."""
import numpy as np

import fp8b_ref
import rowsmx_workers as MW

_mx_case, _mx_rank = MW._case, MW.mx_rank  # (taken at import: the GPU tests put fp8b_rank in MW.mx_rank's place)


class Shape(MW.Shape):
    def expect(self, seed, q, mseed=None):  # (a rowcount that is no multiple of 128 is refused and has no blocks: recv stays FILL)
        return np.full(self.recv_bytes(q), MW.FILL, np.uint8) if self.rowcount % 128 else super().expect(seed, q, mseed)


def _case(comm, case, rank, n, st, barrier):
    """rowsmx_workers._case with the new entry under the name it calls; bad "mxfp8": rank 1 keeps the MXFP8 entry (refused on every rank)."""
    entry = "all_to_all_v_rows_mxfp8" if case.get("bad") == "mxfp8" and rank == 1 else "all_to_all_v_rows_fp8_block128"
    comm.all_to_all_v_rows_mxfp8 = getattr(type(comm), entry).__get__(comm)
    return _mx_case(comm, case, rank, n, st, barrier)


def fp8b_rank(*args, **kw):
    MW._case, MW.Shape, MW.mx_ref = _case, Shape, fp8b_ref  # (in the rank's own process) this file's case, shape and reference
    return _mx_rank(*args, **kw)
