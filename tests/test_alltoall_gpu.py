"""ncclAllToAll on the GPU (-m gpu): the HIP path through the C ABI against the permutation itself,
byte for byte.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  Block r of rank q's recv must be block q of rank r's send: seeded random
bytes, different per rank and call (alltoall_workers.block), so NaN payloads, denormals and every
bit pattern cross.  After every call of every case: the 256 guard bytes past recv and the send are
unchanged, and ipc_open_failures == read_map_failures == 0.
"""
import os

import pytest

import alltoall_workers as AW
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


def _case(dtype="f32", count=4099, algo=READ, **kw):
    return dict(dtype=dtype, count=count, algo=algo, **kw)


def _other(coll, dtype="f32", op="sum", count=4099, inplace=False, algo=READ, root=0, **kw):
    return dict(coll=coll, dtype=dtype, op=op, count=count, inplace=inplace, algo=algo, root=root, **kw)


def _run(n, cases, env=None, timeout=240):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(AW.a2a_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
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
    """n = 3, every supported dtype: 4099 elements per block (a vector body plus a scalar tail), 1 and
    2, 1001 and 1003 halves (1003: odd block bytes, the scalar path), 4100 halves on a 2-byte-misaligned
    base (the scalar path).  last_algo: 0 on the ring, 2 on read."""
    cases = []
    for dt in DTYPES:
        for count in (4099, 1, 2):
            cases.append(_case(dt, count, algo, seed=11 + len(cases)))
    for dt in ("f16", "bf16"):
        for count in (1001, 1003):
            cases.append(_case(dt, count, algo, seed=11 + len(cases)))
    cases.append(_case("f16", 4100, algo, seed=11 + len(cases), offset=2))
    _run(3, cases)


# 2. exchange shapes -------------------------------------------------------------------------------
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}
NS = [2, 3, 5, 8, 9]  # exchange_push has one form for every rank count; 9: past the 8 of a node


@pytest.mark.parametrize("n", NS)
def test_shapes_default_geometry(dev, n):
    """count = 2^20 + 5 f32 and bf16 per block at the defaults: 4 MiB blocks, several batches per slice
    and a short last vector (f32); bf16's block bytes are no multiple of 4: the element path at size."""
    _run(n, [_case("f32", (1 << 20) + 5, READ, seed=21), _case("bf16", (1 << 20) + 5, READ, seed=22)], timeout=300)


@pytest.mark.parametrize("n", NS)
def test_shapes_small_slices(dev, n):
    """1 KiB slices on 4 pipelines, 300 and 16411 elements per block: at least 16 iterations per
    pipeline at 16411, the last slice short."""
    cases = [_case(dt, count, READ, seed=25 + i) for i, (dt, count) in
             enumerate([("f32", 300), ("f32", 16411), ("bf16", 300), ("bf16", 16411)])]
    _run(n, cases, env=SMALL)


# 3. composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,blocking", [(RING, "1"), (READ, "1"), (AUTO, "1"), (RING, "0"), (READ, "0"), (AUTO, "0")])
def test_transpose_twice_is_the_identity(dev, algo, blocking):
    """Two all-to-alls in a row, the first's recv fed as the second's send into a third buffer, return
    every rank's original buffer; 3 rounds on one communicator."""
    n, port = 4, GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    out = GW.run_ranks(AW.transpose_twice_rank, n, lambda r: (r, n, port, e, algo, 17501, 3), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [[0, 0]] * 3 and o["destroy"] == 0 and o["async"] == 0, (r, o)
        assert o["bad_mid"] == [0, 0, 0] and o["bad_back"] == [0, 0, 0] and o["bad_guard"] == [0, 0, 0], (r, o)
        want = 0 if algo == RING else 2
        assert o["algos"] == [(want, want)] * 3, (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 4. interleaving ----------------------------------------------------------------------------------
def test_interleaved_collectives_on_one_communicator(dev):
    """14 calls on one communicator mixing all six collectives on both schedules, sizes alternating,
    every rank entering every call 0-30 ms out of step, every call checked: the FIFO counters the
    schedules share stay in step (the ring's all-to-all advances each link by n(n-1)/2 per iteration)."""
    sk = dict(skew_ms=30)
    cases = [
        _case(count=50001, algo=AUTO, **sk),
        _other("rd", count=4099, algo=READ, root=3, **sk),
        _case(count=300, algo=RING, **sk),
        _other("ag", count=70001, algo=RING, **sk),
        _case(count=70001, algo=RING, dtype="f64", **sk),
        _other("bc", count=300, algo=RING, root=2, inplace=True, **sk),
        _case(count=3, algo=READ, dtype="bf16", **sk),
        _other("ar", count=1024, algo=ONESHOT, expect_algo=3, **sk),
        _case(count=1, algo=RING, **sk),
        _other("rs", count=300, algo=READ, inplace=True, **sk),
        _case(count=100003, algo=READ, **sk),
        _other("rd", count=70001, algo=RING, root=0, inplace=True, null=True, **sk),
        _other("ar", count=40000, algo=RING, expect_algo=0, **sk),
        _case(count=4099, algo=AUTO, dtype="i32", **sk),
    ]
    _run(4, [dict(c, seed=40 + i) for i, c in enumerate(cases)])


# 5. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_ring(dev, mem):
    """Pinned memory through its device mapping, pageable memory through the staging buffer (both
    buffers pageable: staged side by side), a placement per rank, and send and recv placed
    differently: under auto the ring on every rank, exact, two calls per case."""
    cases = [_case("f32", 20011, AUTO, mem=mem, expect_algo=0, seed=50, calls=2),
             _case("bf16", 1001, AUTO, mem=mem, expect_algo=0, seed=51, calls=2),
             _case("f32", 4099, AUTO, mem="device", recv_mem=mem, expect_algo=0, seed=52, calls=2),
             _case("f64", 4099, AUTO, mem=mem, recv_mem="device", expect_algo=0, seed=53, calls=2)]
    _run(3, cases)


# 6. cached consumer -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_pushes_visible_to_a_plain_load_consumer(dev, n):
    port = GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    count = (512 << 10) // 4 // n  # 512 KiB per rank
    out = GW.run_ranks(AW.consumer_rank, n, lambda r: (r, n, port, e, count, 4), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 7. refused calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("overlap", [4, 4, 4]), ("same", [4, 4]), ("null", [4, 4]), ("dtype", [3]),
                                           ("kinds", [5])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidArgument (4) for any overlap of the two buffers, send == recv included, and for a
    NULL buffer; ncclInternalError (3) for ncclInt8; ncclInvalidUsage (5) on both ranks when rank 0
    calls ncclAllToAll where rank 1 calls ncclAllGather with the same count -- without a hang, with
    nothing written, mncclCommGetAsyncError 0, and the communicator's next two valid calls exact."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(AW.errors_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["touched"] == 0, (r, scenario, o)
        assert o["async_after"] == 0 and o["next_rc"] == [0, 0] and o["next_bad"] == 0, (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0
