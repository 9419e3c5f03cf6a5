"""mncclAllToAllvCombine without a GPU (-m "not gpu"): the local checks of csrc/combine.h, one hand-made
case per verdict in the order they are made, and an idle rank that is accepted."""
import ctypes

import pytest

import sim_alltoallv_api as V

SZ = ctypes.c_size_t
OK, TOPK, ZERO_ROW, STRIDE, TOO_MANY, NULL, OVERFLOW, RECV_OVERLAP, SEND_RECV = range(9)
S, R, I, W, TOP = 0x10000, 0x80000, 0x40000, 0x48000, (1 << 64) - 1
C, D, Z = [4, 0, 7], [0, 4, 4], [0, 0, 0]
BASE = dict(esz=2, s=S, sc=C, sd=D, r=R, nrows=100, stride=12, idx=I, w=W, topk=2, rc=C, rd=D, rowcount=10)
EXT = (99 * 12 + 10) * 2  # the recv matrix's byte extent


@pytest.mark.parametrize("want,change", [
    (OK, {}),
    (OK, dict(w=None)),                                                    # NULL weights: every weight 1
    (OK, dict(s=None, r=None, idx=None, w=None, sc=Z, rc=Z, nrows=0)),     # an idle rank
    (OK, dict(r=None, idx=None, nrows=0)),                                 # only serves its send
    (OK, dict(s=None, sc=Z)),                                              # only pulls
    (TOPK, dict(topk=0)), (TOPK, dict(topk=17, stride=9)),                 # before everything else
    (ZERO_ROW, dict(rowcount=0, stride=0)), (ZERO_ROW, dict(rowcount=0, stride=0, sc=Z, rc=Z)),  # nrows alone
    (OK, dict(rowcount=0, stride=0, sc=Z, rc=Z, nrows=0)),
    (STRIDE, dict(stride=9, s=None)),                                      # before the NULL check
    (TOO_MANY, dict(nrows=1 << 30)), (OK, dict(nrows=(1 << 30) - 1, r=1 << 50)),
    (NULL, dict(s=None)), (NULL, dict(r=None)), (NULL, dict(idx=None)),
    (OVERFLOW, dict(rowcount=1 << 30, stride=1 << 30)),                    # a row of 2 GiB
    (OVERFLOW, dict(sd=[TOP - 2, 0, 4])), (OVERFLOW, dict(rd=[TOP, 0, 4])), (OVERFLOW, dict(stride=TOP // 2 + 1)),
    (OVERFLOW, dict(idx=TOP - 20)), (OVERFLOW, dict(w=TOP - 20)),
    (RECV_OVERLAP, dict(rd=[0, 4, 3])), (OK, dict(sd=[0, 0, 0])),          # send blocks may overlap: only read
    (SEND_RECV, dict(r=S + 11 * 20 - 1)), (OK, dict(r=S + 11 * 20)),       # the last send block's last byte; adjacent
    (SEND_RECV, dict(r=S - EXT + 1)), (OK, dict(r=S - EXT)),
    (SEND_RECV, dict(r=I + 800 - 1)), (OK, dict(r=I + 800)),               # slotidx: nrows * topk * 4 bytes
    (SEND_RECV, dict(r=W - EXT + 1)), (OK, dict(r=W - EXT + 1, w=None)),   # weights, unless NULL
])
def test_local_checks_in_order(sim_lib, want, change):
    a = dict(BASE, **change)
    arr = [(SZ * 3)(*a[k]) for k in ("sc", "sd", "rc", "rd")]
    got = V.load().mnccl_sim_combine_check_local(
        3, a["esz"], ctypes.c_void_p(a["s"]), arr[0], arr[1], ctypes.c_void_p(a["r"]), SZ(a["nrows"]), SZ(a["stride"]),
        ctypes.c_void_p(a["idx"]), ctypes.c_void_p(a["w"]), a["topk"], arr[2], arr[3], SZ(a["rowcount"]))
    assert got == want
