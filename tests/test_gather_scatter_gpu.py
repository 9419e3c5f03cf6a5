"""ncclGather / ncclScatter on the GPU (-m gpu): the HIP path through the C ABI against the
permutation itself, computed with numpy -- byte for byte, no tolerance.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  Blocks are seeded random bytes (NaN payloads included); every buffer sits
between 256 sentinel bytes before it and after it; a non-root's unused large buffer is NULL in half
the cases and a sentinel buffer, which must come back unchanged, in the other half
(gather_scatter_workers.GSCall).
"""
import os

import pytest

import gather_scatter_workers as W
import gpu_workers as GW

pytestmark = pytest.mark.gpu

RING, READ, ONESHOT, AUTO = 0, 2, 3, -1
ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}
NDEV = [1]


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    NDEV[0] = out[0]["count"]
    return NDEV[0]


def _case(coll, dtype="f32", count=4099, inplace=False, algo=READ, root=0, **kw):
    return dict(coll=coll, dtype=dtype, count=count, inplace=inplace, algo=algo, root=root, **kw)


def _spawn(target, n, args, timeout=240):
    port = GW.free_port()
    out = GW.run_ranks(target, n, lambda r: (r, n, port) + tuple(args), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0, (r, out[r])
    return out


def _run(n, cases, env=None, timeout=240):
    e = dict(ENV, **(env or {}))
    out = _spawn(W.cases_rank, n, (cases, e), timeout)
    colo = GW.colocated(dict(os.environ, **e))
    for r in range(n):
        info = out[r]["info"]
        assert info["device"] == GW.rank_device(r, NDEV[0], colo), (r, info["device"])
        assert len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches {res['detail']}"
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
@pytest.mark.parametrize("root", [0, 1, 2])
@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_matrix(dev, algo, root):
    """n = 3, every root, f16 / f32 / f64, out of place and in place on the root: 4099 elements per
    block (vector body plus element tail), 1003 halves (odd block bytes: the element path), 4100
    halves on a 2-byte-misaligned base (the element path)."""
    cases = []

    def add(coll, dt, count, inplace, **kw):
        # NULL for the unused buffer in half the cases, a sentinel buffer in the other half
        cases.append(_case(coll, dt, count, inplace, algo, root, null=len(cases) % 2 == 0, seed=11 + len(cases), **kw))
    for inplace in (False, True):
        for coll in ("ga", "sc"):
            for dt in ("f16", "f32", "f64"):
                add(coll, dt, 4099, inplace)
            add(coll, "f16", 1003, inplace)
            add(coll, "f16", 4100, inplace, offset=2)
    _run(3, cases)


# 2. shapes at the default geometry ----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_shapes_default_geometry(dev, n):
    """Blocks of 2^20 + 5 f32 elements at the defaults, the read schedule, roots 0 and n - 1: more than
    one batch in every slice, the last slice short and ending in an element tail."""
    count = (1 << 20) + 5
    cases = []
    for i, root in enumerate((0, n - 1)):
        cases += [_case("ga", "f32", count, i == 1, READ, root, seed=21 + i, null=i == 0),
                  _case("sc", "f32", count, i == 0, READ, root, seed=23 + i, null=i == 1)]
    _run(n, cases, timeout=300)


# 3. small slices ----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
@pytest.mark.parametrize("n", [2, 5, 8])
def test_shapes_small_slices(dev, n, algo):
    """1 KiB slices on 4 pipelines: blocks of 300 elements and of 16411 (16 and more iterations per
    pipeline, the last slice short), roots 0 and n - 1, two calls each: the second finds the counters
    where the first left them."""
    cases = []
    for root in (0, n - 1):
        for count in (300, 16411):
            cases += [_case("ga", "f32", count, count == 300, algo, root, seed=25, null=True, calls=2),
                      _case("sc", "f32", count, count != 300, algo, root, seed=26, calls=2)]
    _run(n, cases, env=SMALL)


# 4. identities ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,blocking", [(RING, "1"), (READ, "1"), (RING, "0"), (READ, "0")])
def test_identities(dev, algo, blocking):
    """On one communicator, 3 rounds: gather then scatter from the same root returns every rank's
    input; the root's gather result equals its ncclAllGather result; rank q's scatter result equals
    block q of what ncclBroadcast of the root's send delivers."""
    n = 4
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    out = _spawn(W.identities_rank, n, (e, algo, 17501, 3))
    for r in range(n):
        o = out[r]
        assert o["rcs"] == [[0] * 5] * 3 and o["async"] == 0, (r, o)
        assert o["round_trip_bad"] == [0, 0, 0], (r, o)
        assert o["gather_vs_allgather"] == [0, 0, 0] and o["scatter_vs_broadcast"] == [0, 0, 0], (r, o)
        assert o["algos"] == [(algo, algo)] * 3, (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 5. interleaving ----------------------------------------------------------------------------------
def test_interleaved_collectives_on_one_communicator(dev):
    """12 calls on one communicator mixing gather and scatter with the other collectives on both
    schedules, the root changing from call to call, sizes alternating, every rank entering every call
    0-30 ms out of step: the FIFO counters the schedules share stay in step (the ring's chains advance
    each link by what it carried, which differs from link to link)."""
    sk = dict(skew_ms=30)
    cases = [
        _case("ga", count=50001, algo=AUTO, root=1, null=True, **sk),
        dict(_case("rd", count=4099, algo=READ, root=3, **sk), op="sum"),
        _case("sc", count=70001, algo=RING, root=2, **sk),
        dict(_case("ag", count=300, algo=RING, **sk), op="sum"),
        _case("ga", count=300, algo=RING, root=3, inplace=True, **sk),
        dict(_case("ar", count=40000, algo=RING, expect_algo=0, **sk), op="sum"),
        _case("sc", count=3, algo=RING, root=0, inplace=True, null=True, **sk),
        dict(_case("a2a", count=1001, algo=READ, **sk), op="sum"),
        _case("ga", count=1, algo=RING, root=0, **sk),
        dict(_case("bc", count=300, algo=RING, root=2, null=True, **sk), op="sum"),
        _case("sc", count=100003, algo=READ, root=3, dtype="f64", **sk),
        _case("ga", count=4099, algo=READ, root=2, dtype="f16", **sk),
    ]
    _run(4, [dict(c, seed=40 + i) for i, c in enumerate(cases)])


# 6. visibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["ga", "sc"])
@pytest.mark.parametrize("n", [2, 4])
def test_pushes_visible_to_a_plain_load_consumer(dev, n, coll):
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    count = (512 << 10) // 4  # 512 KiB per block
    out = _spawn(W.consumer_rank, n, (e, coll, count, 4))
    for r in range(n):
        o = out[r]
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 7. graphs ----------------------------------------------------------------------------------------
def test_graph_capture_and_replay(dev):
    """n = 3: a captured gather and a captured scatter on device buffers, on the read schedule and on
    the ring (whose own-block copy must be captured too), out of place and in place, each replayed 3
    times with inputs changed between replays.  A pageable buffer under capture is ncclInvalidUsage,
    and eager calls afterwards are right."""
    n = 3
    cases = [dict(coll=coll, algo=algo, root=root, count=4099, inplace=inplace, seed=300 + 10 * i)
             for i, (coll, algo, root, inplace) in enumerate([("ga", READ, 1, False), ("sc", READ, 2, False),
                                                              ("ga", RING, 0, False), ("sc", RING, 1, False),
                                                              ("ga", READ, 2, True), ("sc", RING, 0, True)])]
    out = _spawn(W.graph_rank, n, (ENV, cases, 3))
    for r in range(n):
        o = out[r]
        assert len(o["results"]) == len(cases)
        for x in o["results"]:
            c = x["case"]
            assert x["capture_rc"] == [0] and x["captured_algo"] == c["algo"], (r, c, x)
            assert x["bad"] == [0, 0, 0], (r, c, x["bad"], x["detail"])
            assert x["async"] == 0 and x["ipc_open_failures"] == 0 and x["read_map_failures"] == 0, (r, c, x)
        assert o["refused"] == [5, 5], (r, o["refused"])  # ncclInvalidUsage
        assert [(e[0], e[1]) for e in o["eager"]] == [(0, 0), (0, 0)], (r, o["eager"])
        assert [e[2] for e in o["eager"]] == [[RING], [READ]], (r, o["eager"])
        assert o["async"] == 0


# 8. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_ring(dev, mem):
    """Pinned memory through its device mapping, pageable memory through the staging buffer in the
    in-place layout, and a placement per rank: the ring on every rank, exact."""
    cases = []
    for i, (coll, inplace, root) in enumerate([("ga", False, 0), ("ga", True, 2), ("sc", False, 1), ("sc", True, 2),
                                               ("ga", False, 1), ("sc", False, 0)]):
        cases.append(_case(coll, "f32" if i < 4 else "f16", 20011 if i < 4 else 1003, inplace, AUTO, root, mem=mem,
                           expect_algo=0, seed=50 + i, calls=2, null=i % 2 == 0))
    _run(3, cases)


# 9. refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("root", [5, 5]), ("kinds", [5]), ("range", [4, 4, 4, 4]),
                                           ("null", [4, 4, 4, 4]), ("overlap", [4, 4, 4]), ("dtype", [3, 3]),
                                           ("group", [5, 5])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidUsage (5) when the ranks disagree on the root or call gather against scatter,
    ncclInvalidArgument (4) for a root out of range, a needed NULL buffer and a partial overlap on the
    root, ncclInternalError (3) for ncclInt8, ncclInvalidUsage (5) inside an open group -- on every
    rank, without a hang, and the communicator's next valid calls are right."""
    n = 2
    out = _spawn(W.errors_rank, n, (ENV, scenario), timeout=120)
    for r in range(n):
        o = out[r]
        assert o["rcs"] == want, (r, scenario, o)
        if scenario == "group":
            assert o["group_start"] == 0 and o["group_end"] == 0, (r, o)
        assert o["async_after"] == 0 and o["next_rc"] == [0, 0] and o["next_bad"] == [0, 0], (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0, (r, o)


# 10. windows --------------------------------------------------------------------------------------
def test_buffers_in_registered_windows_are_negotiated(dev):
    """MINI_NCCL_WINDOW_RENDEZVOUS=0, n = 3: between two window all-reduces (window_calls + 1 each), a
    gather and a scatter whose buffers lie in the registered windows, out of place and in place, are
    negotiated like any other call: exact, the read schedule, window_calls unchanged."""
    e = dict(ENV, MINI_NCCL_WINDOW_RENDEZVOUS="0")
    out = _spawn(W.windows_rank, 3, (e,))
    what = ["ar@window", "ga@window", "sc@window", "ga@window", "sc@window", "ar@window"]
    for r in range(3):
        o = out[r]
        assert o["windows"] == 2 and o["deregister"] == [0, 0] and o["async"] == 0, (r, o)
        assert [s["what"] for s in o["steps"]] == what
        for s in o["steps"]:
            assert s["rc"] == 0 and s["bad"] == 0 and s["algo"] == 2, (r, s)
            assert s["window_calls"] == (1 if s["what"] == "ar@window" else 0), (r, s)
