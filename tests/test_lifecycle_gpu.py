"""ncclReduceScatter, ncclAllGather, ncclBroadcast, ncclReduce and ncclAllToAll ("the five") on the
paths around the data path (-m gpu): HIP graph capture and replay, ranks as threads of one process,
a communicator of one rank, calls chained across two streams without a host wait, ncclCommDestroy
with calls in flight, buffers inside registered windows, send and recv inside one allocation, and
MINI_NCCL_SYS_FENCE=1 -- what include/mini_nccl_ext.h promises for them "as ncclAllReduce", which
tests/test_gpu.py checks for the all-reduce alone.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  Every check is exact (lifecycle_workers.Call.check): arithmetic results
against the oracle bit for bit (NaN payloads of + and * excepted), copies byte for byte, the 256
guard bytes past each recv, the send where the call only reads it, and a sentinel-filled buffer in
place of the side a rooted call's non-root does not use; mncclCommGetAsyncError == 0,
ncclCommDestroy == 0 and ipc_open_failures == read_map_failures == 0.
"""
import os

import pytest

import alltoall_workers as AW
import gpu_workers as GW
import lifecycle_workers as LW

pytestmark = pytest.mark.gpu

RING, READ, AUTO = 0, 2, -1
SCHEDULES = [pytest.param(RING, id="ring"), pytest.param(READ, id="read")]
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


def _spawn(target, n, args, env, timeout=240):
    """n rank processes of `target(rank, n, port, env, *args, out_q, barrier=)`; every rank reported,
    none raised, nothing failed to map, no asynchronous error, destroy succeeded."""
    port = GW.free_port()
    out = GW.run_ranks(target, n, lambda r: (r, n, port, env) + tuple(args), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        o = out[r]
        assert "error" not in o, f"rank {r}:\n{o['error']}"
        assert o["destroy"] == 0, (r, o["destroy"])
        if "info" in o:
            _check_placement(r, n, o["info"], env)
        for x in [o] + list(o.get("results", [])):
            if "async" in x:
                assert x["async"] == 0 and x["ipc_open_failures"] == 0 and x["read_map_failures"] == 0, (r, x)
    return out


# 1. graph capture and replay ----------------------------------------------------------------------
REPLAYS = 4


def _graph_case(coll, algo, layout="separate", seed=100):
    """21851 elements per rank or block: a vector body, a scalar tail and more than one slice on the
    ring; 3 * 21851 + 2 for the rooted calls: a short last chunk.  Root 1; rank 0 passes NULL for
    the buffer its role does not use, rank 2 a sentinel-filled buffer."""
    count = 3 * 21851 + 2 if coll in ("bc", "rd") else 21851
    return dict(coll=coll, algo=algo, count=count, root=1, null_ranks=[0], layout=layout, seed=seed)


def _run_graph(cases):
    out = _spawn(LW.graph_rank, 3, (cases, REPLAYS), ENV)
    for r in range(3):
        assert len(out[r]["results"]) == len(cases)
        for x in out[r]["results"]:
            c = x["case"]
            assert x["capture_rc"] == [0], (r, c, x["capture_rc"])
            assert x["captured_algo"] == c["algo"], (r, c, x["captured_algo"])
            assert x["bad"] == [0] * REPLAYS, f"rank {r} case {c}: mismatches per replay {x['bad']}: {x['detail']}"
            assert x["eager_rc"] == 0 and x["eager_bad"] == 0 and x["eager_algo"] == c["algo"], (r, c, x["eager_detail"])
            assert x["ar_rc"] == 0 and x["ar_bad"] == 0 and x["last_algo"] == c["algo"], (r, c, x["ar_detail"])


@pytest.mark.parametrize("algo", SCHEDULES)
@pytest.mark.parametrize("coll", LW.FIVE)
def test_graph_capture_and_replay(dev, coll, algo):
    """One out-of-place call captured (n = 3, f32), replayed 4 times with new seeded inputs and a
    refilled recv before every replay: a pre-launch copy (the ring's own chunk, own block, root's
    own copy) that was not captured, or peer pointers or counters baked in at capture time, leave
    the fill bytes or an earlier replay's data in the own chunk, own block or root data.  Then an
    eager call of the same collective and an eager ncclAllReduce: the counters are still in step."""
    _run_graph([_graph_case(coll, algo)])


def test_graph_capture_and_replay_in_place(dev):
    """The read schedule's in-place forms captured and replayed, one after the other on one
    communicator: rs and ag in place as NCCL defines it, bc and rd in place on the root."""
    _run_graph([_graph_case(coll, READ, "inplace", seed=150 + i) for i, coll in enumerate(("rs", "ag", "bc", "rd"))])


@pytest.mark.parametrize("algo", [pytest.param(AUTO, id="auto"), pytest.param(RING, id="ring")])
@pytest.mark.parametrize("pair", LW.PAIRS)
def test_graph_pairs(dev, pair, algo):
    """Two calls captured into ONE graph (n = 4, 4 x 4099 f32), 3 replays with new inputs: rs then
    ag, and rd then bc from root 2, give the all-reduce's bits on every rank; a2a then a2a returns
    the original buffer."""
    out = _spawn(LW.graph_pair_rank, 4, (pair, algo, 4099, 2, 3), ENV)
    want = 0 if algo == RING else 2
    for r in range(4):
        o = out[r]
        assert o["capture"] == [(0, want), (0, want)], (r, o["capture"])
        assert o["bad"] == [0, 0, 0], f"rank {r}: mismatches per replay {o['bad']}: {o['detail']}"


# 2. ranks as threads of one process ---------------------------------------------------------------
def _thread_cases(n):
    """Each of the five on both schedules, out of place and in the in-place forms that exist, 4099
    f32 and 1001 bf16 (odd chunk bytes: the scalar path); rooted calls with roots 0 and n - 1, NULL on
    odd non-root ranks and a sentinel buffer on even ones (lifecycle_workers._call_of)."""
    cases = []
    for dtype, count in (("f32", 4099), ("bf16", 1001)):
        for algo in (RING, READ):
            for layout in ("separate", "inplace"):
                cases += [dict(coll=coll, algo=algo, dtype=dtype, count=count, layout=layout) for coll in ("rs", "ag")]
                cases += [dict(coll=coll, algo=algo, dtype=dtype, count=count, layout=layout, root=root)
                          for coll in ("bc", "rd") for root in (0, n - 1)]
            cases.append(dict(coll="a2a", algo=algo, dtype=dtype, count=count))
    return cases


def _run_threads(n, cases, env, timeout=300):
    port = GW.free_port()
    out = GW.run_ranks(LW.threaded_colls_proc, 1, lambda _: (n, port, env, cases), timeout)
    assert 0 in out and "error" not in out[0], out
    ranks = out[0]["ranks"]
    assert sorted(ranks) == list(range(n)), ranks
    for r in range(n):
        o = ranks[r]
        assert "error" not in o, o["error"]
        assert o["ranks_on_device"] == n and o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0, (r, o)
        assert o["destroy"] == 0 and len(o["results"]) == len(cases), (r, o)
        for x in o["results"]:
            assert x["rc"] == 0 and x["bad"] == 0 and x["async"] == 0, (r, x)
            assert x["last_algo"] == x["case"]["algo"], (r, x)


@pytest.mark.parametrize("n", [2, 3])
def test_ranks_as_threads(dev, n):
    """The same-process peer paths (raw pointers in one address space, no dma-buf) for the five: the
    stand-in buffers of a rooted call's non-roots and root_relay's in-place test compare raw
    addresses here."""
    _run_threads(n, _thread_cases(n), ENV)


def test_sixteen_ranks_as_threads(dev):
    """The largest communicator on the GPU: each of the five once on read and once on ring, 4099 f32
    per rank or block; bc / rd with count 16 * 257 + 3 and root 5 (chunks of 258, a short last chunk),
    bc also in place on the root (relay_peer's skip-the-root rotation in its loop form)."""
    cases = []
    for algo in (READ, RING):
        cases += [dict(coll=coll, algo=algo, count=4099) for coll in ("rs", "ag", "a2a")]
        cases += [dict(coll=coll, algo=algo, count=16 * 257 + 3, root=5) for coll in ("bc", "rd")]
        cases.append(dict(coll="bc", algo=algo, count=16 * 257 + 3, root=5, layout="inplace"))
    _run_threads(16, cases, {"MINI_NCCL_TIMEOUT_MS": "60000", "GPU_MAX_HW_QUEUES": "16"})


# 3. one rank --------------------------------------------------------------------------------------
def test_one_rank_is_a_copy(dev):
    """nranks == 1: each of the five is the copy of its whole buffer (nranks * count elements for
    the halves and the all-to-all), out of place and in place (recv == send), on device and pageable
    host buffers, 4099 elements and 1; no kernel launches (last_algo stays -1).  ncclAllToAll with
    send == recv or a partial overlap is ncclInvalidArgument here too, count == 0 is ncclSuccess for
    all five, and neither writes anything."""
    cases = []
    for coll, dtype in zip(LW.FIVE, ("f32", "f64", "i32", "f16", "bf16")):
        for count in (4099, 1):
            for mem in ("device", "pageable"):
                for layout in ("separate",) if coll == "a2a" else ("separate", "inplace"):
                    cases.append(dict(coll=coll, dtype=dtype, count=count, mem=mem, layout=layout))
    port = GW.free_port()
    out = GW.run_ranks(LW.one_rank_proc, 1, lambda _: (port, ENV, cases), 120)
    assert 0 in out and "error" not in out[0], out
    o = out[0]
    assert len(o["results"]) == len(cases)
    for x in o["results"]:
        assert x["rc"] == 0 and x["bad"] == 0 and x["last_algo"] == -1, x
    assert o["refused"] == [4, 4, 4] and o["zero"] == [0] * 5 and o["touched"] == 0, o
    assert o["last_algo"] == -1 and o["async"] == 0 and o["destroy"] == 0, o
    assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0, o


# 4. calls chained across two streams --------------------------------------------------------------
@pytest.mark.parametrize("algo", SCHEDULES + [pytest.param(AUTO, id="auto")])
def test_chains_across_two_streams(dev, algo):
    """MINI_NCCL_BLOCKING=0, n = 3, two rounds of three chains, 12 calls with no host wait until the
    end, consecutive calls on alternating streams, each second call reading what the first wrote:
    rs into X then ag from X (the all-reduce's bits), rd to root 1 then bc from root 1 (3 x 17500
    elements), a2a then a2a of its recv (the original).  Without the communicator's cross-stream
    ordering the second call of a chain reads the fill bytes."""
    out = _spawn(LW.chains_rank, 3, (algo, 2), dict(ENV, MINI_NCCL_BLOCKING="0"))
    want = 0 if algo == RING else 2
    for r in range(3):
        o = out[r]
        assert o["calls"] == [(0, want)] * 12, (r, o["calls"])
        assert o["bad"] == [0] * 6, f"rank {r}: mismatches per chain {o['bad']}: {o['detail']}"


# 5. destroy with calls in flight ------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["ring", "read"])
def test_destroy_waits_for_calls_in_flight(dev, algo):
    """rs, bc from root 2 and a2a at 1 Mi f32 elements each queued with MINI_NCCL_BLOCKING=0, then
    ncclCommDestroy at once: it waits for them, and all three results are complete."""
    env = dict(ENV, MINI_NCCL_BLOCKING="0", MINI_NCCL_ALGO=algo)
    port = GW.free_port()
    out = GW.run_ranks(LW.destroy_inflight_rank, 3, lambda r: (r, 3, port, env, 1 << 20), 240, barrier=True)
    assert sorted(out) == [0, 1, 2], out
    want = 0 if algo == "ring" else 2
    for r in range(3):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0, 0, 0] and o["algos"] == [want] * 3 and o["destroy"] == 0, (r, o)
        assert o["bad"] == [0, 0, 0], (r, o["bad"], o["detail"])
        assert o["async"] == 0 and o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0, (r, o)


# 6. buffers inside registered windows -------------------------------------------------------------
def test_five_between_window_allreduces(dev):
    """MINI_NCCL_WINDOW_RENDEZVOUS=0, n = 3: window all-reduces publish fast records on the board the
    five's negotiated calls use, with the same call counter.  A window all-reduce, the five on
    sub-ranges of the windows, a window all-reduce, the five outside any window, a window all-reduce:
    window_calls goes up by exactly 1 at each all-reduce and by 0 at each of the others, the read
    schedule throughout."""
    out = _spawn(LW.windows_rank, 3, (), dict(ENV, MINI_NCCL_WINDOW_RENDEZVOUS="0"))
    five = list(LW.FIVE)
    what = (["ar@window"] + [c + "@window" for c in five] + ["ar@window"] + [c + "@outside" for c in five] + ["ar@window"])
    for r in range(3):
        o = out[r]
        assert o["windows"] == 2 and o["windows_after"] == 0 and o["deregister"] == [0, 0], (r, o)
        assert [s["what"] for s in o["steps"]] == what
        for s in o["steps"]:
            assert s["rc"] == 0 and s["bad"] == 0 and s["async"] == 0 and s["algo"] == 2, (r, s)
            assert s["window_calls"] == (1 if s["what"] == "ar@window" else 0), (r, s)


# 7. send and recv in one allocation ---------------------------------------------------------------
def test_send_and_recv_in_one_allocation(dev):
    """One hipMalloc per rank and case, send and recv at disjoint offsets 256 bytes apart, the read
    schedule, two calls each: the first maps one descriptor for both buffers (one mapping round),
    the second needs none.  bc with the root out of place: its two mapped addresses differ only by
    the offset.  Rank 0 passes a sentinel region of the same allocation for the side a rooted call
    does not use, rank 2 NULL."""
    cases = [dict(coll=coll, algo=READ, count=3 * 4099 + 2 if coll in ("bc", "rd") else 4099, root=1, null_ranks=[2],
                  layout="one", calls=2) for coll in LW.FIVE]
    out = _spawn(LW.cases_rank, 3, (cases,), ENV)
    for r in range(3):
        assert len(out[r]["results"]) == len(cases)
        for x in out[r]["results"]:
            assert x["rcs"] == [0, 0] and x["bad"] == [0, 0] and x["algos"] == [2, 2], (r, x)
            assert x["rounds"] == [1, 0], (r, x["case"], x["rounds"])


# 8. system fences ---------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", SCHEDULES)
def test_sys_fence_on(dev, algo):
    """MINI_NCCL_SYS_FENCE=1: read_half's fence branches and the ring's for the five's op kinds; 4099
    f32 and 1001 bf16, rd and rs with Sum and Max (alltoall_workers.a2a_rank's eager runners)."""
    cases = []
    for dtype, count in (("f32", 4099), ("bf16", 1001)):
        for coll, op, root in (("rs", "sum", 0), ("rs", "max", 0), ("ag", "sum", 0), ("bc", "sum", 1), ("rd", "sum", 2),
                               ("rd", "max", 0), ("a2a", "sum", 0)):
            cases.append(dict(coll=coll, dtype=dtype, op=op, count=count, inplace=False, algo=algo, root=root,
                              null=coll == "rd", seed=60 + len(cases)))
    env = dict(ENV, MINI_NCCL_SYS_FENCE="1")
    port = GW.free_port()
    out = GW.run_ranks(AW.a2a_rank, 3, lambda r: (r, 3, port, cases, env), 240, barrier=True)
    assert sorted(out) == [0, 1, 2], f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(3):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0 and out[r]["info"]["sys_fence"] == 1, (r, out[r]["info"])
        _check_placement(r, 3, out[r]["info"], env)
        assert len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
            assert res["async"] == 0 and res["algos"] == [algo], (r, c, res)
            assert res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0, (r, c, res)
