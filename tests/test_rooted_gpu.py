"""ncclBroadcast / ncclReduce on the GPU (-m gpu): the HIP path through the C ABI against the CPU
oracle, bit for bit (NaN payloads of + and * excepted, as for the all-reduce).

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  A Broadcast's every rank must hold the root's input; a Reduce's root
rooted_ref.reduce_expect (chunks of ceil(count / n) elements, each folded in the all-reduce's order
for that chunk), and nobody else's recv may be touched.  Every call of every case is checked, 256
guard bytes past each recv included; a non-root passes NULL for the buffer its role does not use in
half the cases and a filled buffer, which must come back unchanged, in the other half.
"""
import os

import pytest

import gpu_workers as GW
import rooted_workers as RW

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


def _case(coll, dtype="f32", op="sum", count=4099, inplace=False, algo=READ, root=0, **kw):
    return dict(coll=coll, dtype=dtype, op=op, count=count, inplace=inplace, algo=algo, root=root, **kw)


def _run(n, cases, env=None, timeout=240):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(RW.rooted_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
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
@pytest.mark.parametrize("root", [0, 1, 2])
@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_matrix(dev, algo, root):
    """n = 3, every root, Reduce over every dtype x op and Broadcast over every dtype, out of place and
    in place on the root: 4099 elements (vector body, a scalar tail, a short last chunk), 1001 and
    1003 halves (1003: odd chunk bytes, the scalar path), 4100 halves on a 2-byte-misaligned base (the
    scalar path), 2 elements (one chunk is empty), 1 element, and f32 / f64 special values."""
    cases = []

    def add(coll, dt, op, count, inplace, **kw):
        # NULL for the unused buffer in half the cases, a filled buffer in the other half
        cases.append(_case(coll, dt, op, count, inplace, algo, root, null=len(cases) % 2 == 0, **kw))
    for inplace in (False, True):
        for dt in DTYPES:
            for op in OPS:
                add("rd", dt, op, 4099, inplace, seed=11)
            add("bc", dt, "sum", 4099, inplace, seed=12)
            for count in (2, 1):
                add("rd", dt, "sum", count, inplace, seed=13)
                add("bc", dt, "sum", count, inplace, seed=14)
        for dt in ("f16", "bf16"):
            for count in (1001, 1003):
                for op in OPS:
                    add("rd", dt, op, count, inplace, seed=15)
                add("bc", dt, "sum", count, inplace, seed=16)
        for op in OPS:
            add("rd", "f16", op, 4100, inplace, seed=17, offset=2)
        add("bc", "f16", "sum", 4100, inplace, seed=18, offset=2)
        for dt in ("f32", "f64"):
            for op in OPS:
                add("rd", dt, op, 4099, inplace, seed=19, special=True)
            add("bc", dt, "sum", 4099, inplace, seed=20, special=True)
    _run(3, cases)


# 2. fold and relay shapes -------------------------------------------------------------------------
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}


@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_shapes_default_geometry(dev, n):
    """root_fold's fold and root_relay's pushes at G = 1, 2, 4, 7 descriptor slots and in the loop
    past 8 ranks: count = n * 2^20 + 5 at the defaults (4 MiB chunks, more than one batch per slice at
    every G, a last chunk unlike the others), f32 and bf16 Sum, roots 0 and n - 1."""
    count = n * (1 << 20) + 5
    cases = []
    for i, root in enumerate((0, n - 1)):
        cases += [_case("rd", "f32", "sum", count, i == 1, READ, root, seed=21, null=i == 0),
                  _case("rd", "bf16", "sum", count, i == 0, READ, root, seed=22, null=i == 1),
                  _case("bc", "f32", "sum", count, i == 0, READ, root, seed=23, null=i == 0),
                  _case("bc", "bf16", "sum", count, i == 1, READ, root, seed=24, null=i == 1)]
    _run(n, cases, timeout=300)


@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_shapes_small_slices(dev, n):
    """The same with 1 KiB slices on 4 pipelines: 300 elements and 16411 (16 and more iterations per
    pipeline, the last slice short), roots 0 and n - 1."""
    cases = []
    for root in (0, n - 1):
        for dt in ("f32", "bf16"):
            for count in (300, 16411):
                cases += [_case("rd", dt, "sum", count, False, READ, root, seed=25, null=True),
                          _case("rd", dt, "sum", count, True, READ, root, seed=26),
                          _case("bc", dt, "sum", count, count == 300, READ, root, seed=27, null=count != 300),
                          _case("bc", dt, "sum", count, count != 300, READ, root, seed=28)]
    _run(n, cases, env=SMALL)


# 3. composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,blocking", [(RING, "1"), (READ, "1"), (AUTO, "1"), (RING, "0"), (READ, "0"), (AUTO, "0")])
def test_reduce_then_broadcast_is_all_reduce(dev, algo, blocking):
    """count = 4 * 17500: the Reduce's result on the root is ncclAllReduce's, bit for bit, and
    Reduce then Broadcast gives it on every rank; 3 rounds on one communicator."""
    n, port = 4, GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    out = GW.run_ranks(RW.compose_rank, n, lambda r: (r, n, port, e, algo, 4 * 17500, 3), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [[0, 0, 0]] * 3 and o["destroy"] == 0 and o["async"] == 0, (r, o)
        assert o["root_bad_vs_allreduce"] == [0, 0, 0], (r, o)
        assert o["bad_vs_allreduce"] == [0, 0, 0] and o["bad_vs_oracle"] == [0, 0, 0], (r, o)
        want = 0 if algo == RING else 2
        assert all(a[0] == want and a[1] == want for a in o["algos"]), (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 4. interleaving ----------------------------------------------------------------------------------
def test_interleaved_collectives_on_one_communicator(dev):
    """12 calls on one communicator mixing all five collectives on both schedules, the root changing
    from call to call, sizes alternating, every rank entering every call 0-30 ms out of step: the
    FIFO counters the schedules share stay in step (the ring's Broadcast advances each link by what
    it carried)."""
    sk = dict(skew_ms=30)
    cases = [
        _case("bc", count=50001, algo=AUTO, root=1, null=True, **sk),
        _case("rd", count=4099, algo=READ, root=3, **sk),
        _case("ag", count=70001, algo=RING, **sk),
        _case("bc", count=300, algo=RING, root=2, inplace=True, **sk),
        _case("ar", count=1024, algo=ONESHOT, expect_algo=3, **sk),
        _case("rd", count=70001, algo=RING, root=0, inplace=True, null=True, **sk),
        _case("rs", count=300, algo=READ, inplace=True, **sk),
        _case("bc", count=3, algo=RING, root=3, **sk),
        _case("rd", count=300, algo=AUTO, root=2, dtype="bf16", **sk),
        _case("ar", count=40000, algo=RING, expect_algo=0, **sk),
        _case("rd", count=1, algo=RING, root=1, null=True, **sk),
        _case("bc", count=100003, algo=READ, root=0, dtype="f64", **sk),
    ]
    _run(4, [dict(c, seed=40 + i) for i, c in enumerate(cases)])


# 5. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_ring(dev, mem):
    """Pinned memory through its device mapping, pageable memory through the staging buffer (the
    root stages in and the others out for a Broadcast; everyone in and the root out for a Reduce),
    and a placement per rank: the ring on every rank, exact."""
    cases = []
    for i, (coll, inplace, root) in enumerate([("rd", False, 0), ("rd", True, 2), ("bc", False, 1), ("bc", True, 2)]):
        cases.append(_case(coll, "f32", "sum", 20011, inplace, AUTO, root, mem=mem, expect_algo=0, seed=50 + i, calls=2,
                           null=i % 2 == 0))
    # send and recv placed differently (one on the device, the other on the host)
    cases.append(_case("rd", "f32", "max", 4099, False, AUTO, 1, mem="device", recv_mem=mem, expect_algo=0, seed=55, calls=2))
    # (a Broadcast reads the root's send only: rank 1's is on the host in every parametrisation)
    cases.append(_case("bc", "bf16", "sum", 1001, False, AUTO, 1, mem=mem, recv_mem="device", expect_algo=0, seed=56,
                       calls=2))
    _run(3, cases)


# 6. cached consumer -------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["bc", "rd"])
@pytest.mark.parametrize("n", [2, 4])
def test_pushes_visible_to_a_plain_load_consumer(dev, n, coll):
    port = GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    count = (512 << 10) // 4  # 512 KiB
    out = GW.run_ranks(RW.consumer_rank, n, lambda r: (r, n, port, e, coll, count, 4), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 7. errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("root", [5, 5]), ("kinds", [5]), ("range", [4, 4, 4, 4]),
                                           ("null", [4, 4, 4, 4]), ("overlap", [4, 4]), ("dtype", [3, 3])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidUsage (5) when the ranks disagree on the root or on the collective,
    ncclInvalidArgument (4) for a root out of range, a NULL buffer the rank's role needs and a
    partial overlap on the root, ncclInternalError (3) for an unsupported datatype -- on every rank,
    without a hang, and the communicator's next valid calls are right."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(RW.errors_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["async_after"] == 0 and o["next_rc"] == [0, 0] and o["next_bad"] == 0, (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0 and o["destroy"] == 0, (r, o)
