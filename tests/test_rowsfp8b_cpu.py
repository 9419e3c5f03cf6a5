"""mncclAllToAllvRowsFp8Block128 without a GPU: csrc/fp8block.h through the simulator against fp8b_ref and hand-made cases."""
import ctypes

import numpy as np
import pytest

import fp8b_ref
import sim_alltoallv_api as V

SZ, U64 = ctypes.c_size_t, ctypes.c_uint64
OK, RECV_OVERLAP, SEND_RECV, MX_ROWCOUNT, MX_ALIGN = 0, 6, 7, 16, 17


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
def test_host_quantiser_matches_the_reference_on_every_pattern(sim_lib, f16):
    rows = fp8b_ref.sweep(f16).reshape(-1, 1024)
    out = np.zeros((rows.shape[0], 1056), np.uint8)
    assert V.load().mnccl_sim_fp8b_quantise(rows.ctypes.data_as(ctypes.c_void_p), int(f16), 1024, U64(rows.shape[0]),
                                            out.ctypes.data_as(ctypes.c_void_p)) == 0
    exp = fp8b_ref.quantise(rows, f16)
    assert np.array_equal(out, exp), np.argwhere(out != exp)[:4]
    scales = np.ascontiguousarray(exp[:, 1024:]).view("<u4")
    floor = (np.float32(1e-4) / np.float32(448)).view(np.uint32)
    assert (scales == 0x7FC00000).any() and (scales == floor).any() and (exp[:, :1024] == 0x7E).any() and (exp[:, :1024] == 0xFE).any()  # NaN / inf blocks, clamped blocks, +-448


@pytest.mark.parametrize("rowcount", [128, 1152])
def test_every_record_is_owned_by_exactly_one_slice(sim_lib, rowcount):  # the record is MXFP8's size: its simulator entry
    assert V.load().mnccl_sim_fp8b_record_bytes(U64(rowcount)) == rowcount + rowcount // 32 == V.load().mnccl_sim_mx_record_bytes(U64(rowcount))
    for count in (0, 2, 40):
        owners = np.zeros(max(count, 1), np.uint32)
        assert V.load().mnccl_sim_mx_owners(U64(count), U64(40), U64(rowcount), U64(1024), owners.ctypes.data_as(ctypes.c_void_p)) == 0
        assert (owners[:count] == 1).all(), (count, owners)


@pytest.mark.parametrize("kw,verdict", [
    ({}, OK), (dict(rowcount=16384, stride=16384), OK), (dict(rowcount=96, stride=20000), MX_ROWCOUNT),
    (dict(rowcount=16512, stride=20000), MX_ROWCOUNT), (dict(r=0x1000002), MX_ALIGN), (dict(rd=(0, 4, 3)), RECV_OVERLAP),
    (dict(s=0x1000000 + 11 * 1056), OK), (dict(s=0x1000000 + 11 * 1056 - 4), SEND_RECV)])  # overlap counted in P = 1056 bytes a record
def test_local_checks(sim_lib, kw, verdict):
    def chk(s=0x10000, stride=1030, idx=0x800000, sc=(4, 0, 7), r=0x1000000, rc=(4, 0, 7), rd=(0, 4, 4), rowcount=1024):
        a = [(SZ * 3)(*x) for x in (sc, (0, 4, 4), rc, rd)]
        return V.load().mnccl_sim_fp8b_check_local(3, 2, ctypes.c_void_p(s), SZ(100), SZ(stride), ctypes.c_void_p(idx), a[0], a[1],
                                                   ctypes.c_void_p(r), a[2], a[3], SZ(rowcount))
    assert chk(**kw) == verdict
