"""ncclAllToAllv on the GPU (-m gpu): the HIP path through the C ABI against the permutation itself,
byte for byte.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  Elements [sd[r][q], +C[r][q]) of rank r's send must be elements
[rd[q][r], +C[r][q]) of rank q's recv: seeded random bytes, different per rank, pair and call
(alltoall_workers.block).  After every call of every case: the gaps between the recv blocks, the
256 guard bytes past recv and the send are unchanged, and ipc_open_failures == read_map_failures == 0.
"""
import os

import numpy as np
import pytest

import alltoallv_workers as VW
import gpu_workers as GW

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64", "i32", "f16", "bf16"]
RING, READ, ONESHOT, AUTO = 0, 2, 3, -1
ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}
NDEV = [1]


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    NDEV[0] = out[0]["count"]
    return NDEV[0]


def _check_placement(r, n, info, env):
    colo = GW.colocated(dict(os.environ, **env))
    assert info["device"] == GW.rank_device(r, NDEV[0], colo), (r, info["device"])
    assert info["ranks_on_device"] == GW.ranks_sharing_device(r, n, NDEV[0], colo), (r, n, NDEV[0])


def _case(C, dtype="f32", algo=READ, mode="contig", **kw):
    return dict(C=np.array(C).tolist(), dtype=dtype, algo=algo, mode=mode, **kw)


def _other(coll, dtype="f32", op="sum", count=4099, inplace=False, algo=READ, root=0, **kw):
    return dict(coll=coll, dtype=dtype, op=op, count=count, inplace=inplace, algo=algo, root=root, **kw)


def _pattern(n, values, shift=0):
    """C[r][q] = values[(2 r + q + shift) mod len]: neighbours differ, every value occurs from 2 ranks on."""
    return [[values[(2 * r + q + shift) % len(values)] for q in range(n)] for r in range(n)]


def _run(n, cases, env=None, timeout=240):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(VW.v_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        _check_placement(r, n, out[r]["info"], e)
        assert len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
            assert res["async"] == 0
            assert res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0, (r, c, res)
            if "expect_algo" in c:
                want = c["expect_algo"]
            else:
                dev_bufs = all(c.get(k, "device") == "device" for k in ("mem", "recv_mem"))
                # device buffers run the read schedule under read / auto; everything else the ring
                want = 2 if dev_bufs and c["algo"] in (READ, AUTO) else 0
            assert res["algos"] == [want] * c.get("calls", 1), f"rank {r} case {c}: ran schedules {res['algos']}"
    return out


# 1. the matrix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_matrix(dev, algo):
    """n = 3, every supported dtype, counts from {0, 1, 2, 4099} spread so that no rank's row or
    column repeats a neighbour (4099: a vector body plus a scalar tail; an empty block; blocks shorter
    than a vector), displacements contiguous, then reversed with 3-element gaps.  last_algo: 0 on the
    ring, 2 on read."""
    C = [[1, 4099, 0], [2, 0, 4099], [4099, 1, 2]]
    cases = [_case(C, dt, algo, mode, seed=11 + i) for i, (dt, mode) in
             enumerate((dt, mode) for dt in DTYPES for mode in ("contig", "gaps"))]
    _run(3, cases)


# 2. slices running out at different times ---------------------------------------------------------
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}


@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_slices_run_out_at_different_times(dev, n):
    """1 KiB slices on 4 pipelines, per-pair counts from {0, 300, 16411}: at 16411 the call has at
    least 16 iterations per pipeline, during most of which the 300-element and empty destinations are
    already exhausted; f32 and bf16 (16411 halves: block bytes no multiple of 4)."""
    cases = [_case(_pattern(n, (16411, 0, 300), i), dt, READ, ("contig", "gaps")[i % 2], seed=25 + i)
             for i, dt in enumerate(("f32", "bf16", "f32"))]
    _run(n, cases, env=SMALL)


def test_one_large_block_at_the_default_geometry(dev):
    """One block of 2^20 + 5 elements (4 MiB: several batches per slice, a short last vector) among
    empty and tiny ones at the default geometry: the whole call's slices follow that one block."""
    n = 4
    C = np.zeros((n, n), dtype=np.int64)
    C[2, 1] = (1 << 20) + 5
    C[0, 3], C[1, 1], C[3, 0] = 1, 3, 7
    _run(n, [_case(C, "f32", READ, "gaps", seed=31), _case(C.T, "bf16", READ, "contig", seed=32)], timeout=300)


# 3. mixed alignment -------------------------------------------------------------------------------
def _parity_displs(counts, odd):
    """Non-overlapping displacements, block q starting at an odd element where odd[q], else even."""
    d, at = [], 0
    for c, o in zip(counts, odd):
        at += (at % 2) != int(o)
        d.append(at)
        at += int(c) + 1
    return d


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mixed_alignment_in_one_call(dev, dtype):
    """2-byte elements, n = 3: every rank sends to one destination from an odd displacement and to the
    others from even ones, receives from one source at an odd displacement, and rank 1's send and rank
    0's recv sit on a base that is itself 2 bytes off -- so in ONE call some destinations are
    dword-aligned on both sides (16-byte path) and others are not (element path).  Block bytes that
    are multiples of neither 16 nor 4 (1003 and 9 halves) and of 4 but not 16 (4098)."""
    n = 3
    C = np.array([[9, 1003, 4098], [4098, 9, 1003], [1003, 4098, 9]])
    sd = [_parity_displs(C[r, :], [q == (r + 1) % n for q in range(n)]) for r in range(n)]
    rd = [_parity_displs(C[:, r], [q == (r + 2) % n for q in range(n)]) for r in range(n)]
    cases = [_case(C, dtype, READ, sd=sd, rd=rd, seed=35, calls=2),
             _case(C, dtype, READ, sd=sd, rd=rd, seed=36, offset=[0, 2, 0], recv_offset=[2, 0, 0]),
             _case(C, dtype, RING, sd=sd, rd=rd, seed=37, offset=[0, 2, 0], recv_offset=[2, 0, 0])]
    _run(n, cases)


# 4. agreement with ncclAllToAll -------------------------------------------------------------------
def test_uniform_counts_agree_with_alltoall(dev):
    """Uniform counts with contiguous displacements: byte-identical recv to ncclAllToAll on the same send."""
    n = 4
    cases = [_case(np.full((n, n), c), dt, algo, vs_a2a=True, seed=38 + i)
             for i, (dt, c, algo) in enumerate([("f32", 4099, READ), ("bf16", 1003, READ), ("f32", 4099, RING)])]
    _run(n, cases)


# 5. idle ranks ------------------------------------------------------------------------------------
def test_idle_ranks_and_an_all_zero_matrix(dev):
    """An all-zero matrix returns 0, launches nothing (last_algo still -1) and writes nothing.  Then
    rank 1 with all-zero counts and both buffers NULL still takes part, and every rank -- the idle
    one too -- runs the read schedule."""
    n = 4
    C = np.array(_pattern(n, (300, 4099, 17)))
    C[1, :] = 0
    C[:, 1] = 0
    cases = [_case(np.zeros((n, n), dtype=int), "f32", READ, null_ranks=[0, 1, 2, 3], expect_algo=-1, seed=41),
             _case(C, "f32", READ, "gaps", null_ranks=[1], seed=42, calls=2),
             _case(C, "bf16", AUTO, "contig", null_ranks=[1], seed=43)]
    _run(n, cases)


# 6. round trip ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,blocking", [(RING, "1"), (READ, "1"), (AUTO, "1"), (RING, "0"), (READ, "0"), (AUTO, "0")])
def test_round_trip_returns_every_block(dev, algo, blocking):
    n, port = 4, GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    C = _pattern(n, (17501, 0, 3, 4099, 300))
    out = GW.run_ranks(VW.round_trip_rank, n, lambda r: (r, n, port, e, algo, C, 3), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [[0, 0]] * 3 and o["destroy"] == 0 and o["async"] == 0, (r, o)
        assert o["bad_mid"] == [0, 0, 0] and o["bad_back"] == [0, 0, 0] and o["bad_guard"] == [0, 0, 0], (r, o)
        want = 0 if algo == RING else 2
        assert o["algos"] == [(want, want)] * 3, (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 7. interleaving ----------------------------------------------------------------------------------
def test_interleaved_with_the_six_other_collectives(dev):
    """13 calls on one communicator mixing ncclAllToAllv with the six other collectives on both
    schedules, every rank entering every call 0-30 ms out of step, every call checked: the counters
    the schedules share stay in step (a variable call advances them as an all-to-all of its largest
    block does)."""
    n, sk = 4, dict(skew_ms=30)
    P = lambda vals, s=0: _pattern(n, vals, s)
    cases = [
        _case(P((50001, 0, 7)), algo=AUTO, mode="gaps", **sk),
        _other("rd", count=4099, algo=READ, root=3, **sk),
        _case(P((300, 1, 0, 17)), algo=RING, **sk),
        _other("ag", count=70001, algo=RING, **sk),
        dict(coll="a2a", dtype="f64", count=3001, algo=READ, **sk),
        _case(P((3, 0), 1), algo=READ, dtype="bf16", **sk),
        _other("bc", count=300, algo=RING, root=2, inplace=True, **sk),
        _case(P((70001, 5, 0), 2), algo=RING, dtype="f64", mode="gaps", **sk),
        _other("ar", count=1024, algo=ONESHOT, expect_algo=3, **sk),
        _case(P((100003, 0, 0, 1)), algo=READ, **sk),
        _other("rs", count=300, algo=READ, inplace=True, **sk),
        dict(coll="a2a", dtype="f32", count=300, algo=RING, **sk),
        _case(P((4099, 1003)), algo=AUTO, dtype="i32", mode="reversed", **sk),
    ]
    _run(n, [dict(c, seed=40 + i) for i, c in enumerate(cases)])


# 8. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_padded_ring(dev, mem):
    """Pinned and pageable host memory, a placement per rank, and send and recv placed differently:
    the copies of the padded fallback read and write them directly; under auto the ring on every
    rank, exact, two calls per case."""
    n = 3
    C = _pattern(n, (20011, 0, 1001, 3))
    cases = [_case(C, "f32", AUTO, "gaps", mem=mem, expect_algo=0, seed=50, calls=2),
             _case(C, "bf16", AUTO, mem=mem, expect_algo=0, seed=51, calls=2),
             _case(C, "f32", AUTO, mem="device", recv_mem=mem, expect_algo=0, seed=52, calls=2),
             _case(C, "f64", AUTO, "reversed", mem=mem, recv_mem="device", expect_algo=0, seed=53, calls=2)]
    _run(n, cases)


# 9. refused calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("null_array", [4, 4, 4, 4]), ("recv_overlap", [4, 4]), ("send_recv", [4, 4, 4]),
                                           ("dtype", [3]), ("mismatch", [5]), ("kinds", [5])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidArgument (4) for a NULL array, overlapping recv blocks and a recv block overlapping
    a send block; ncclInternalError (3) for ncclInt8; ncclInvalidUsage (5) on both ranks for a
    one-element count mismatch and when rank 0 calls ncclAllToAllv where rank 1 calls ncclAllToAll --
    without a hang, with nothing written, mncclCommGetAsyncError 0, and the communicator's next two
    valid calls exact."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(VW.errors_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["touched"] == 0, (r, scenario, o)
        assert o["async_after"] == 0 and o["next_rc"] == [0, 0] and o["next_bad"] == 0, (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 10. graphs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [pytest.param(READ, id="read"), pytest.param(RING, id="ring")])
def test_graph_capture(dev, algo):
    """A read-schedule call captured and replayed 3 times with fresh data, exact; a forced-ring call
    under capture is ncclInvalidUsage on every rank and the communicator stays usable (the eager call
    after it is exact)."""
    n, port = 3, GW.free_port()
    C = _pattern(n, (4099, 0, 300, 20011))
    out = GW.run_ranks(VW.graph_rank, n, lambda r: (r, n, port, ENV, algo, C, 3), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        if algo == READ:
            assert o["capture_rc"] == [0] and o["captured_algo"] == 2 and o["bad"] == [0, 0, 0], (r, o)
        else:
            assert o["capture_rc"] == [5] and o["bad"] == [], (r, o)
        assert o["eager_rc"] == 0 and o["eager_bad"] == 0 and o["eager_algo"] == algo, (r, o)
        assert o["async"] == 0 and o["destroy"] == 0
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 11. cached consumer ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_pushes_visible_to_a_plain_load_consumer(dev, n):
    port = GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    per = (512 << 10) // 4 // n  # about 512 KiB per rank, unevenly split
    C = _pattern(n, (per, per // 2 + 3, per + per // 2 + 1))
    out = GW.run_ranks(VW.consumer_rank, n, lambda r: (r, n, port, e, C, 4), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 12. one rank -------------------------------------------------------------------------------------
def test_one_rank(dev):
    """nranks == 1: a copy of block 0 from sdispls[0] to rdispls[0] whatever the schedule setting; a
    count mismatch is ncclInvalidUsage (5) and an all-zero call succeeds, both writing nothing."""
    port = GW.free_port()
    out = GW.run_ranks(VW.one_rank, 1, lambda r: (port, ENV), 120)
    assert sorted(out) == [0], out
    o = out[0]
    assert "error" not in o, o.get("error")
    assert o["rcs"] == [0, 0, 5, 0] and o["bad"] == [0, 0, 0, 0], o
    assert o["async"] == 0 and o["destroy"] == 0
