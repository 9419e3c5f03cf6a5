"""ncclReduceScatter / ncclAllGather on the GPU (-m gpu): the HIP path through the C ABI against
the CPU oracle, bit for bit (NaN payloads of + and * excepted, as for the all-reduce).

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  A reduce-scatter's rank r must hold chunk r of the oracle's ring fold
(the all-reduce's bits); an all-gather's every rank the concatenation of the inputs.  Every call of
every case is checked, 256 guard bytes past each recv included.  Counts are per rank.
"""
import os

import pytest

import coll_workers as CW
import gpu_workers as GW

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f64", "i32", "f16", "bf16"]
OPS = ["sum", "prod", "max", "min"]
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


def _case(coll, dtype="f32", op="sum", count=4099, inplace=False, algo=READ, **kw):
    return dict(coll=coll, dtype=dtype, op=op, count=count, inplace=inplace, algo=algo, **kw)


def _run(n, cases, env=None, timeout=240):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(CW.coll_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
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
    """n = 3, every dtype x op, both collectives, out of place and in place: 4099 elements (vector
    body + a scalar tail of len % 16), 1001 halves (odd chunk bytes: the scalar path), 4100 halves on
    a 2-byte-misaligned base (the scalar path), 1 element, and f32 / f64 special values."""
    cases = []
    for inplace in (False, True):
        for dt in DTYPES:
            cases += [_case("rs", dt, op, 4099, inplace, algo, seed=11) for op in OPS]
            cases.append(_case("ag", dt, "sum", 4099, inplace, algo, seed=12))
            cases.append(_case("rs", dt, "sum", 1, inplace, algo, seed=13))
            cases.append(_case("ag", dt, "sum", 1, inplace, algo, seed=14))
        for dt in ("f16", "bf16"):
            cases += [_case("rs", dt, op, 1001, inplace, algo, seed=15) for op in OPS]
            cases.append(_case("ag", dt, "sum", 1001, inplace, algo, seed=16))
        cases += [_case("rs", "f16", op, 4100, inplace, algo, seed=17, offset=2) for op in OPS]
        cases.append(_case("ag", "f16", "sum", 4100, inplace, algo, seed=18, offset=2))
        for dt in ("f32", "f64"):
            cases += [_case("rs", dt, op, 4099, inplace, algo, seed=19, special=True) for op in OPS]
            cases.append(_case("ag", dt, "sum", 4099, inplace, algo, seed=20, special=True))
    _run(3, cases)


# 2. fold shapes -----------------------------------------------------------------------------------
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}


@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_fold_shapes_default_geometry(dev, n):
    """The read schedule's fold at G = 1, 2, 4, 7 peer slots and past 8 ranks: 4 MiB chunks at the
    defaults (16 KiB slices: more than one batch per slice at every G), f32 and bf16 Sum."""
    count = (1 << 20) + 5
    _run(n, [_case("rs", "f32", "sum", count, False, READ, seed=21),
             _case("rs", "bf16", "sum", count, True, READ, seed=22),
             _case("ag", "f32", "sum", count, False, READ, seed=23)], timeout=300)


@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_fold_shapes_small_slices(dev, n):
    """The same folds with 1 KiB slices on 4 pipelines: 300 elements (two slices, the last short) and
    16411 (about 64 KiB chunks: 16 iterations per pipeline, last slice short)."""
    cases = []
    for dt in ("f32", "bf16"):
        for count in (300, 16411):
            cases += [_case("rs", dt, "sum", count, False, READ, seed=24), _case("rs", dt, "sum", count, True, READ, seed=25),
                      _case("ag", dt, "sum", count, count == 300, READ, seed=26)]
    _run(n, cases, env=SMALL)


# 3. composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,blocking", [(RING, "1"), (READ, "1"), (AUTO, "1"), (AUTO, "0")])
def test_reduce_scatter_then_all_gather_is_all_reduce(dev, algo, blocking):
    n, port = 4, GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    out = GW.run_ranks(CW.compose_rank, n, lambda r: (r, n, port, e, algo, 70001, 3), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [[0, 0, 0]] * 3 and o["destroy"] == 0 and o["async"] == 0, (r, o)
        assert o["bad_vs_allreduce"] == [0, 0, 0] and o["bad_vs_oracle"] == [0, 0, 0], (r, o)
        half = 0 if algo == RING else 2
        assert all(a[0] == half and a[1] == half for a in o["algos"]), (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 4. interleaving ----------------------------------------------------------------------------------
def test_interleaved_collectives_on_one_communicator(dev):
    """12 calls on one communicator: all-reduces (auto, ring, one-shot-sized) between reduce-scatters
    and all-gathers on both schedules, sizes alternating, every rank entering every call 0-30 ms out
    of step: the FIFO counters the schedules share stay in step."""
    sk = dict(skew_ms=30)
    cases = [
        _case("ar", count=50001, algo=AUTO, expect_algo=2, **sk),
        _case("rs", count=4099, algo=READ, **sk),
        _case("ag", count=70001, algo=RING, **sk),
        _case("ar", count=1024, algo=ONESHOT, expect_algo=3, **sk),
        _case("rs", count=70001, algo=RING, inplace=True, **sk),
        _case("ag", count=300, algo=READ, inplace=True, **sk),
        _case("ar", count=40000, algo=RING, expect_algo=0, **sk),
        _case("ag", count=4099, algo=AUTO, **sk),
        _case("rs", count=300, algo=AUTO, dtype="bf16", **sk),
        _case("ar", count=300, algo=READ, expect_algo=2, inplace=True, **sk),
        _case("rs", count=1, algo=RING, **sk),
        _case("ag", count=100003, algo=READ, dtype="f64", **sk),
    ]
    _run(4, [dict(c, seed=40 + i) for i, c in enumerate(cases)])


# 5. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_ring(dev, mem):
    """Pinned memory through its device mapping, pageable memory through the staging buffer in the
    in-place layout, and a placement per rank: the ring on every rank, exact."""
    cases = []
    for i, (coll, inplace) in enumerate([("rs", False), ("rs", True), ("ag", False), ("ag", True)]):
        cases.append(_case(coll, "f32", "sum", 20011, inplace, AUTO, mem=mem, expect_algo=0, seed=50 + i, calls=2))
    # recv placed differently from send (send on the device, recv on the host)
    cases.append(_case("rs", "f32", "max", 4099, False, AUTO, mem="device", recv_mem=mem, expect_algo=0, seed=55))
    cases.append(_case("ag", "bf16", "sum", 1001, False, AUTO, mem=mem, recv_mem="device", expect_algo=0, seed=56))
    _run(3, cases)


# 6. cached consumer -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_all_gather_pushes_visible_to_a_plain_load_consumer(dev, n):
    port = GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    count = (512 << 10) // 4  # 512 KiB per rank
    out = GW.run_ranks(CW.gather_consumer_rank, n, lambda r: (r, n, port, e, count, 4), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 7. errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("overlap", [4, 4]), ("counts", [5]), ("kinds", [5]), ("dtype", [3, 3])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidArgument (4) for a partial overlap, ncclInvalidUsage (5) when the ranks disagree on
    the count or on the collective, ncclInternalError (3) for an unsupported datatype -- on every
    rank, without a hang, and the communicator's next valid call is right."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(CW.errors_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["async_after"] == 0 and o["next_rc"] == 0 and o["next_bad"] == 0, (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0 and o["destroy"] == 0, (r, o)
