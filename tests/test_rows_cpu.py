"""mncclAllToAllvRows without a GPU (-m "not gpu"): the ABI's argument checks, the host-side rules
(csrc/rowblock.h) on hand-made cases, and the simulated rows_push -- every slice, destination and row
walked by the kernel's own unit rule -- against numpy fancy indexing, byte for byte."""
import ctypes
import subprocess

import numpy as np
import pytest

import rows_workers as RW
import sim_alltoallv_api as V

U64, SZ = ctypes.c_uint64, ctypes.c_size_t
OK, ZERO_ROW, STRIDE, TOO_MANY, NULL, OVERFLOW, RECV_OVERLAP, SEND_RECV = range(8)


def test_symbol_and_argument_checks_before_the_communicator_is_read(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    out = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True, check=True)
    assert "mncclAllToAllvRows" in {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
    assert len(M.SIGNATURES["mncclAllToAllvRows"][1]) == 13 and callable(M.Comm.all_to_all_v_rows)
    assert L.mncclVersion() == 600  # detected by symbol, not by version
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)  # never dereferenced on these paths
    arr = (SZ * 2)(4, 4)
    call = lambda comm, sc=arr, sd=arr, rc=arr, rd=arr, dt=M.ncclFloat: \
        L.mncclAllToAllvRows(fake, 8, 4, other, sc, sd, other, rc, rd, 4, dt, comm, None)
    assert call(None) == call(None, dt=M.ncclInt8) == M.ncclInvalidArgument
    for k in ("sc", "sd", "rc", "rd"):
        assert call(fake, dt=M.ncclInt8, **{k: None}) == M.ncclInvalidArgument  # 1. NULL comm / array, before the datatype
    assert L.ncclGroupStart() == 0
    assert call(fake, dt=M.ncclInt8) == M.ncclInvalidUsage  # 2. an open group, before the datatype; it stays clean
    assert L.ncclGroupEnd() == 0
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert call(fake, dt=dt) == M.ncclInternalError  # 3. before the communicator (a fake pointer) is read


def _check(esz, s, nrows, stride, idx, sc, sd, r, rc, rd, rowcount):
    a = [(SZ * len(x))(*x) for x in (sc, sd, rc, rd)]
    return V.load().mnccl_sim_rows_check_local(len(sc), esz, ctypes.c_void_p(s), SZ(nrows), SZ(stride), ctypes.c_void_p(idx),
                                               a[0], a[1], ctypes.c_void_p(r), a[2], a[3], SZ(rowcount))


def test_local_checks_in_order(sim_lib):
    s, i, r, top = 0x10000, 0x40000, 0x80000, (1 << 64) - 1
    c, d, z = [4, 0, 7], [0, 4, 4], [0, 0, 0]
    ok = dict(esz=2, s=s, nrows=100, stride=12, idx=i, sc=c, sd=d, r=r, rc=c, rd=d, rowcount=10)
    chk = lambda **kw: _check(**{**ok, **kw})
    assert chk() == OK and chk(s=None, idx=None, r=None, sc=z, rc=z) == OK  # (an idle rank)
    assert chk(rowcount=0, stride=0) == ZERO_ROW and chk(rowcount=0, stride=0, sc=z, rc=z) == OK
    assert chk(stride=9) == STRIDE and chk(stride=9, s=None) == STRIDE  # before the NULL check
    assert chk(nrows=1 << 31) == TOO_MANY and chk(nrows=(1 << 31) - 1, s=1 << 40) == OK
    assert chk(s=None) == chk(idx=None) == chk(r=None) == NULL and chk(s=None, idx=None, sc=z) == OK
    assert chk(rowcount=1 << 30, stride=1 << 30) == OVERFLOW          # a row of 2 GiB
    assert chk(stride=top // 2 + 1) == chk(sd=[top - 2, 0, 4]) == chk(idx=top - 20) == chk(rd=[top, 0, 4]) == OVERFLOW
    assert chk(rd=[0, 4, 3]) == RECV_OVERLAP and chk(sd=[0, 0, 0]) == OK  # index ranges may overlap
    ext = (99 * 12 + 10) * 2
    assert V.load().mnccl_sim_rows_extent(100, 12, 10, 2) == ext
    assert chk(r=s + ext - 1) == SEND_RECV and chk(r=s + ext) == OK       # the extent's last byte; adjacent
    assert chk(r=i + 4 * 11 - 1) == SEND_RECV and chk(r=i + 4 * 11) == OK  # the used part of rowidx
    assert chk(r=s - 11 * 20 + 1) == SEND_RECV and chk(r=s - 11 * 20) == OK


def test_slice_rule_and_argument_block(sim_lib):
    L, out = V.load(), (ctypes.c_uint32 * 2)()
    units = lambda *a: (L.mnccl_sim_rows_units(*a, out), tuple(out))[1]
    # a 1028-byte row from byte 1020, slice [1024, 2048): vector 0 straddles the cut and is the earlier
    # slice's, vector 1 this slice's first; the row's 4-byte tail (byte 2044) is this slice's too
    assert units(1024, 2048, 1020, 0, 16, 64) == (1, 64) and units(0, 1024, 1020, 0, 16, 64) == (0, 1)
    assert units(1024, 2048, 1020, 1024, 4, 1) == (0, 1) and units(2048, 3072, 1020, 1024, 4, 1) == (1, 1)
    assert units(0, 1024, 0, 0, 16, 0) == (0, 0)  # a row shorter than a vector has none
    args = (U64 * 7)()
    sc, sd, recv, prd = (SZ * 3)(2, 0, 5), (SZ * 3)(0, 0, 1), (U64 * 3)(0x1000, 0x2000, 0x3002), (U64 * 3)(1, 9, 3)
    assert L.mnccl_sim_rows_args(3, 2, U64(0x100), SZ(50), SZ(12), sc, sd, SZ(10), recv, prd, args) == 0
    # bytes, then offsets in the peers' recv; an empty block and an odd destination stay off the vector path
    assert list(args) == [40, 0, 100, 20, 180, 60, 0b001]


@pytest.mark.parametrize("n,esz,rowcount,pad,slice_bytes", [(2, 2, 7, 0, 1024), (2, 2, 514, 5, 1024), (3, 4, 257, 0, 1024),
                                                            (3, 1, 1031, 5, 2048), (3, 8, 64, 0, 16), (2, 2, 1500, 0, 1024)])
def test_sim_rows_exchange_matches_fancy_indexing(sim_lib, n, esz, rowcount, pad, slice_bytes):
    """The GPU suite's shapes and reference (rows_workers.Shape), out-of-range indices included; rank 1's
    matrix at an odd address, so vector and element destinations meet in one exchange."""
    C = np.random.default_rng([n, esz, rowcount]).choice([0, 1, 3, 70], size=(n, n))
    sh = RW.Shape(dict(C=C, esz=esz, rowcount=rowcount, pad=pad, idx="oob"), n)
    xs, idx = [sh.matrix(1, r) for r in range(n)], [sh.rowidx(1, r) for r in range(n)]
    recv = [np.full(sh.recv_bytes(r), RW.FILL, np.uint8) for r in range(n)]
    P = lambda arrs, t: (ctypes.POINTER(t) * n)(*[a.ctypes.data_as(ctypes.POINTER(t)) for a in arrs])
    A = lambda v: (U64 * len(v))(*[int(x) for x in v])
    rc = V.load().mnccl_sim_rows_exchange(
        n, esz, U64(slice_bytes), P(xs, ctypes.c_uint8), A([RW.NROWS] * n), A([sh.stride] * n), P(idx, ctypes.c_int32),
        A(C.reshape(-1)), A(np.reshape(sh.sd, -1)), P(recv, ctypes.c_uint8), A(np.reshape(sh.rd, -1)), U64(rowcount),
        A([0x1000 + 2 * (r == 1) for r in range(n)]), A([0x8000] * n))
    assert rc == 0  # (-3: some byte of a block not stored exactly once)
    assert all(np.array_equal(recv[q], sh.expect(1, q)) for q in range(n))
