"""mncclAllToAllvRowsMxfp8 without a GPU: csrc/mxblock.h through the simulator against mx_ref and hand-made cases."""
import ctypes

import numpy as np
import pytest

import mx_ref
import sim_alltoallv_api as V

SZ = ctypes.c_size_t
OK, STRIDE, NULL, RECV_OVERLAP, SEND_RECV, MX_ROWCOUNT, MX_ALIGN = 0, 2, 4, 6, 7, 16, 17


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
def test_host_quantiser_matches_the_reference_on_every_pattern(sim_lib, f16):
    rows = mx_ref.sweep(f16).reshape(-1, 1024)
    out = np.zeros((rows.shape[0], 1056), np.uint8)
    assert V.load().mnccl_sim_mx_quantise(rows.ctypes.data_as(ctypes.c_void_p), int(f16), 1024, ctypes.c_uint64(rows.shape[0]),
                                          out.ctypes.data_as(ctypes.c_void_p)) == 0
    exp = mx_ref.quantise(rows, f16)
    assert np.array_equal(out, exp), np.argwhere(out != exp)[:4]
    assert (exp[:, 1024:] == 0xFF).any() and (exp[:, :1024] == 0x7E).any()


@pytest.mark.parametrize("rowcount", [128, 1152])
def test_every_record_is_owned_by_exactly_one_slice(sim_lib, rowcount):
    L = V.load()
    for count in (0, 2, 40):
        owners = np.zeros(max(count, 1), np.uint32)
        assert L.mnccl_sim_mx_owners(ctypes.c_uint64(count), ctypes.c_uint64(40), ctypes.c_uint64(rowcount), ctypes.c_uint64(1024),
                                     owners.ctypes.data_as(ctypes.c_void_p)) == 0
        assert (owners[:count] == 1).all(), (count, owners)


def test_local_checks(sim_lib):
    def chk(s=0x10000, stride=1030, idx=0x800000, sc=(4, 0, 7), r=0x1000000, rc=(4, 0, 7), rd=(0, 4, 4), rowcount=1024):
        a = [(SZ * 3)(*x) for x in (sc, (0, 4, 4), rc, rd)]
        return V.load().mnccl_sim_mx_check_local(3, 2, ctypes.c_void_p(s), SZ(100), SZ(stride), ctypes.c_void_p(idx), a[0], a[1],
                                                 ctypes.c_void_p(r), a[2], a[3], SZ(rowcount))
    assert chk() == OK and chk(s=None, idx=None, r=None, sc=(0, 0, 0), rc=(0, 0, 0)) == OK  # (an idle rank)
    assert [chk(rowcount=c, stride=20000) for c in (0, 96, 1000, 16512)] == [MX_ROWCOUNT] * 4 and chk(rowcount=16384, stride=16384) == OK
    assert chk(s=0x10002) == chk(r=0x1000002) == chk(stride=1031) == MX_ALIGN
    assert chk(stride=1022) == STRIDE and chk(r=None) == NULL
    assert chk(rd=(0, 4, 3)) == RECV_OVERLAP
    # the recv side counts P = 1056 bytes per record: a matrix 11 records behind recv is hit by the last block only then
    assert chk(s=0x1000000 + 11 * 1056) == OK and chk(s=0x1000000 + 11 * 1056 - 4) == SEND_RECV
