"""combinemx_workers' case and shape with "1 x 128" FP8 records (fp8b_ref, fp8bc_ref) and the new entries; NaN as NaN."""
import numpy as np

import combinemx_workers as MW
import fp8b_ref
import fp8bc_ref

_mx_case, _mx_rank = MW._case, MW.combinemx_rank  # (taken at import: the GPU tests put combinefp8b_rank in combine_rank's place)


class Shape(MW.Shape):  # (the same record size, rows, bits and slots); sweep: every e4m3 code at fp8bc_ref.SCALES[i % 8] in record i
    def send(self, seed, r):
        self.recs = fp8b_ref.quantise(self.rows(seed, r), False)
        if self.case.get("sweep"):
            self.recs[:, :self.rowcount] = np.tile(np.arange(256, dtype=np.uint8), self.rowcount // 256)
            words = np.repeat(fp8bc_ref.SCALES[np.arange(len(self.recs)) % 8, None], self.rowcount // 128, axis=1)
            self.recs[:, self.rowcount:] = words.astype("<u4").view(np.uint8)
        self.sent = fp8bc_ref.decode(self.recs, self.rowcount)
        return self.sent


def _case(comm, case, rank, n, st, barrier):
    """combinemx_workers._case with the new combine and dispatch under the names it calls; mxfp8_on_1: rank 1 keeps the MXFP8 combine."""
    cls, real = type(comm), type(comm).all_to_all_v_combine_mxfp8
    if not (case.get("mxfp8_on_1") and rank == 1):
        cls.all_to_all_v_combine_mxfp8 = cls.all_to_all_v_combine_fp8_block128
    comm.all_to_all_v_rows_mxfp8 = comm.all_to_all_v_rows_fp8_block128
    try:
        return _mx_case(comm, case, rank, n, st, barrier)
    finally:
        cls.all_to_all_v_combine_mxfp8 = real


def combinefp8b_rank(*args, **kw):
    MW._case, MW.Shape = _case, Shape  # (in the rank's own process) combinemx_workers' rank around this file's case and shape
    return _mx_rank(*args, **kw)
