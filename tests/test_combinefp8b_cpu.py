"""mncclAllToAllvCombineFp8Block128 without a GPU: the symbol, csrc/combinefp8b.h's local checks in order, the host decode-and-fold."""
import ctypes

import numpy as np
import pytest

import combinefp8b_workers as BW
import mxc_ref
import sim_alltoallv_api as V
from test_combinemx_cpu import (BASE, MX_ALIGN, MX_ROWCOUNT, NULL, OK, OVERFLOW, RECV_OVERLAP, SEND_RECV, STRIDE, SZ, TOP, TOPK, P,
                                R, S)  # the MXFP8 combine's verdicts and base case: the records are as long


def test_symbol_is_exported_and_bound(nccl_lib):
    import mini_nccl
    assert hasattr(nccl_lib, "mncclAllToAllvCombineFp8Block128") and len(mini_nccl.SIGNATURES["mncclAllToAllvCombineFp8Block128"][1]) == 15


@pytest.mark.parametrize("want,change", [
    (OK, {}), (MX_ROWCOUNT, dict(rowcount=96, stride=96)), (MX_ROWCOUNT, dict(rowcount=16512, stride=16512)),
    (MX_ALIGN, dict(s=S + 2, topk=17)), (MX_ALIGN, dict(r=R + 2)), (MX_ALIGN, dict(stride=129)), (OK, dict(stride=129, esz=4)),
    (TOPK, dict(topk=17)), (STRIDE, dict(stride=124)), (NULL, dict(s=None)),
    (OVERFLOW, dict(sd=[TOP // 100, 0, 4])), (OK, dict(sd=[TOP // 200, 0, 4], s=0x1000)),  # P bytes per send row, not 256
    (RECV_OVERLAP, dict(rd=[0, 4, 3])), (SEND_RECV, dict(r=S + 11 * P - 4)), (OK, dict(r=S + 11 * P)),  # the last record's end
])
def test_local_checks_in_order(sim_lib, want, change):
    a = dict(BASE, **change)
    arr = [(SZ * 3)(*a[k]) for k in ("sc", "sd", "sc", "rd")]
    assert want == V.load().mnccl_sim_combinefp8b_check_local(
        3, a["esz"], ctypes.c_void_p(a["s"]), arr[0], arr[1], ctypes.c_void_p(a["r"]), SZ(a["nrows"]), SZ(a["stride"]),
        ctypes.c_void_p(0x40000), ctypes.c_void_p(0x48000), a["topk"], arr[2], arr[3], SZ(a["rowcount"]))


@pytest.mark.parametrize("case", [dict(rowcount=256, topk=1, sweep=True, weights=False),
                                  dict(rowcount=256, topk=1, sweep=True, w_const=-0.5), dict(rowcount=384, topk=3)])
def test_host_decode_and_fold(sim_lib, case):
    """One rank, 8 records: all 256 codes at each of the 8 scale words, and a random top-3 case; by bits, NaN as NaN."""
    sh = BW.Shape(dict(case, C=[[8]], dtype="f32", nrows=[64]), 1)
    (slots, w), exp = sh.slots(1, 0), sh.expect(1, 0).reshape(64, -1)
    x = sh.send(1, 0)
    if case.get("sweep"):  # (record i carries scale i % 8: 2^-140 at 2, 2^120 at 3, -0.5 at 4, +inf at 6, NaN at 7)
        assert np.isnan(x[7]).all() and np.isinf(x[3, 126]) and x[4, 126] == -224 and x[2, 1] == np.float32(2.0 ** -149)
        assert np.isnan(x[6, 0]) and x[6, 0x81] == -np.inf
    block, fn = np.ascontiguousarray(sh.recs[sh.sd[0][0]:][:8]), V.load().mnccl_sim_combinefp8b_fold_row
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    for t in range(64):
        got, s = np.zeros(case["rowcount"], np.float32), slots[t] - np.int32(sh.rd[0][0])  # (positions in the block)
        wt = w[t].ctypes.data if sh.weighted else None
        assert fn(block.ctypes.data, 8, case["rowcount"], s.ctypes.data, wt, len(s), got.ctypes.data) == 0
        assert np.array_equal(mxc_ref.canon(got.view(np.uint8), "f32"), exp[t]), t
