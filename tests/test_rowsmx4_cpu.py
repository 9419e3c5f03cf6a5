"""mncclAllToAllvRowsMxfp4 without a GPU: csrc/mxblock.h's mx4_ rules through the simulator against mx4_ref and hand-made cases."""
import ctypes

import numpy as np
import pytest

import mx4_ref
import sim_alltoallv_api as V

SZ, U64 = ctypes.c_size_t, ctypes.c_uint64
OK, STRIDE, NULL, RECV_OVERLAP, SEND_RECV, MX_ROWCOUNT, MX_ALIGN = 0, 2, 4, 6, 7, 16, 17


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
def test_host_quantiser_matches_the_reference_on_every_pattern(sim_lib, f16):
    rows = mx4_ref.sweep(f16).reshape(-1, 1024)
    out = np.zeros((rows.shape[0], 544), np.uint8)
    assert V.load().mnccl_sim_mx4_quantise(rows.ctypes.data_as(ctypes.c_void_p), int(f16), 1024, U64(rows.shape[0]),
                                           out.ctypes.data_as(ctypes.c_void_p)) == 0
    exp = mx4_ref.quantise(rows, f16)
    assert np.array_equal(out, exp), np.argwhere(out != exp)[:4]
    assert [V.load().mnccl_sim_mx4_scale_byte(E) for E in range(256)] == [max(E - 2, 0) for E in range(255)] + [255]
    assert (exp[:, 512:] == 0xFF).any() and {int(c) for c in np.unique(exp[:, :512] & 15)} == set(range(16))  # NaN blocks, every code


@pytest.mark.parametrize("rowcount", range(128, 16384 + 1, 128))
def test_lane_split(sim_lib, rowcount):  # the walk picks a pass's indices out of one batch of 64: rows a pass must divide 64
    g = (ctypes.c_uint32 * 3)()
    V.load().mnccl_sim_mx4_lanes(rowcount, g)
    lanes, rows, passes = g
    assert lanes == min(rowcount // 32, 64) and passes == -(-rowcount // 2048)
    assert rows in (1, 2, 4, 8, 16) and rows * lanes <= 64 < 2 * rows * lanes  # a power of two, and the largest that fits


@pytest.mark.parametrize("rowcount,P4", [(128, 68), (1152, 612)])
def test_every_record_is_owned_by_exactly_one_slice(sim_lib, rowcount, P4):
    assert V.load().mnccl_sim_mx4_record_bytes(U64(rowcount)) == P4  # (fits the default int restype)
    for count in (0, 2, 40):
        owners = np.zeros(max(count, 1), np.uint32)
        assert V.load().mnccl_sim_mx4_owners(U64(count), U64(40), U64(rowcount), U64(1024), owners.ctypes.data_as(ctypes.c_void_p)) == 0
        assert (owners[:count] == 1).all(), (count, owners)


@pytest.mark.parametrize("kw,verdict", [
    ({}, OK), (dict(s=None, idx=None, r=None, sc=(0, 0, 0), rc=(0, 0, 0)), OK), (dict(rowcount=16384, stride=16384), OK),
    (dict(rowcount=0, stride=20000), MX_ROWCOUNT), (dict(rowcount=96, stride=20000), MX_ROWCOUNT),
    (dict(rowcount=1000, stride=20000), MX_ROWCOUNT), (dict(rowcount=16512, stride=20000), MX_ROWCOUNT),
    (dict(s=0x10002), MX_ALIGN), (dict(r=0x1000002), MX_ALIGN), (dict(stride=1031), MX_ALIGN),
    (dict(stride=1022), STRIDE), (dict(r=None), NULL), (dict(rd=(0, 4, 3)), RECV_OVERLAP),
    # the recv side counts P4 = 544 bytes per record: a matrix 11 records behind recv is hit by the last block only then
    (dict(s=0x1000000 + 11 * 544), OK), (dict(s=0x1000000 + 11 * 544 - 4), SEND_RECV)])
def test_local_checks(sim_lib, kw, verdict):
    def chk(s=0x10000, stride=1030, idx=0x800000, sc=(4, 0, 7), r=0x1000000, rc=(4, 0, 7), rd=(0, 4, 4), rowcount=1024):
        a = [(SZ * 3)(*x) for x in (sc, (0, 4, 4), rc, rd)]
        return V.load().mnccl_sim_mx4_check_local(3, 2, ctypes.c_void_p(s), SZ(100), SZ(stride), ctypes.c_void_p(idx), a[0], a[1],
                                                  ctypes.c_void_p(r), a[2], a[3], SZ(rowcount))
    assert chk(**kw) == verdict
