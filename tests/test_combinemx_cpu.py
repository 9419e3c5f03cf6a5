"""mncclAllToAllvCombineMxfp8 without a GPU: the symbol, csrc/combinemx.h's local checks in order, the host decode-and-fold."""
import ctypes

import numpy as np
import pytest

import combinemx_workers as MW
import mxc_ref
import sim_alltoallv_api as V

OK, TOPK, STRIDE, TOO_MANY, NULL, OVERFLOW, RECV_OVERLAP, SEND_RECV, MX_ROWCOUNT, MX_ALIGN = 0, 1, 3, 4, 5, 6, 7, 8, 16, 17
SZ, S, R, TOP, P = ctypes.c_size_t, 0x10000, 0x80000, (1 << 64) - 1, 132  # P: a record's bytes
BASE = dict(esz=2, s=S, sc=[4, 0, 7], sd=[0, 4, 4], r=R, nrows=100, stride=130, topk=2, rd=[0, 4, 4], rowcount=128)


def test_symbol_is_exported_and_bound(nccl_lib):
    import mini_nccl
    assert hasattr(nccl_lib, "mncclAllToAllvCombineMxfp8") and len(mini_nccl.SIGNATURES["mncclAllToAllvCombineMxfp8"][1]) == 15


@pytest.mark.parametrize("want,change", [
    (OK, {}), (MX_ROWCOUNT, dict(rowcount=96, stride=96)), (MX_ROWCOUNT, dict(rowcount=16512, stride=16512)),
    (MX_ROWCOUNT, dict(rowcount=0, topk=0)), (MX_ALIGN, dict(s=S + 2, topk=17)),  # both in front of topk
    (MX_ALIGN, dict(r=R + 2)), (MX_ALIGN, dict(stride=129)), (OK, dict(stride=129, esz=4)),
    (TOPK, dict(topk=17)), (STRIDE, dict(stride=124)), (TOO_MANY, dict(nrows=1 << 30)), (NULL, dict(s=None)),
    (OVERFLOW, dict(sd=[TOP // 100, 0, 4])), (OK, dict(sd=[TOP // 200, 0, 4], s=0x1000)),  # P bytes per send row, not 256
    (RECV_OVERLAP, dict(rd=[0, 4, 3])), (SEND_RECV, dict(r=S + 11 * P - 4)), (OK, dict(r=S + 11 * P)),  # the last record's end
])
def test_local_checks_in_order(sim_lib, want, change):
    a = dict(BASE, **change)
    arr = [(SZ * 3)(*a[k]) for k in ("sc", "sd", "sc", "rd")]
    assert want == V.load().mnccl_sim_combinemx_check_local(
        3, a["esz"], ctypes.c_void_p(a["s"]), arr[0], arr[1], ctypes.c_void_p(a["r"]), SZ(a["nrows"]), SZ(a["stride"]),
        ctypes.c_void_p(0x40000), ctypes.c_void_p(0x48000), a["topk"], arr[2], arr[3], SZ(a["rowcount"]))


@pytest.mark.parametrize("case", [dict(rowcount=256, topk=1, sweep=True, weights=False),
                                  dict(rowcount=256, topk=1, sweep=True, w_const=-0.5), dict(rowcount=384, topk=3)])
def test_host_decode_and_fold(sim_lib, case):
    """One rank, 8 records: all 256 codes at each of the 8 scale bytes, and a random top-3 case; by bits, NaN as NaN."""
    sh = MW.Shape(dict(case, C=[[8]], dtype="f32", nrows=[64]), 1)
    (slots, w), exp = sh.slots(1, 0), sh.expect(1, 0).reshape(64, -1)
    x = sh.send(1, 0)
    if case.get("sweep"):  # (the block's records carry the scale bytes 1 .. 255 and 0, in this order)
        assert np.isnan(x[7]).all() and np.isinf(x[6, 126]) and x[8, 1] == np.float32(2.0 ** -136) and x[4, 126] == 7 * 2.0 ** 125
    block, fn = np.ascontiguousarray(sh.recs[sh.sd[0][0]:][:8]), V.load().mnccl_sim_combinemx_fold_row
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    for t in range(64):
        got, s = np.zeros(case["rowcount"], np.float32), slots[t] - np.int32(sh.rd[0][0])  # (positions in the block)
        wt = w[t].ctypes.data if sh.weighted else None
        assert fn(block.ctypes.data, 8, case["rowcount"], s.ctypes.data, wt, len(s), got.ctypes.data) == 0
        assert np.array_equal(mxc_ref.canon(got.view(np.uint8), "f32"), exp[t]), t
