"""mncclAllGatherv / mncclReduceScatterv on the GPU (-m gpu): the HIP path through the C ABI, the gather
against the permutation itself byte for byte, the fold against the reference fold on block c laid into
chunk c (oracle_api.ring_fold / premul_ref / fp8_ref) bit for bit.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  After every call of every case: the gaps between the blocks, the guards
behind the buffers and the sends are unchanged, ipc_open_failures == read_map_failures == 0, and
window_calls has not moved.  Most tests set 1 KiB slices on 4 pipelines (SMALL), so that blocks of a
few thousand elements span several slices and iterations.
"""
import numpy as np
import pytest

import gpu_workers as GW
import vhalves_workers as HW

pytestmark = pytest.mark.gpu

RING, READ, AUTO = 0, 2, -1
ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}
ESZ = {"f32": 4, "f64": 8, "i32": 4, "f16": 2, "bf16": 2, "e4m3": 1, "e5m2": 1}


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    return out[0]["count"]


def _case(coll, counts, dtype="f32", op="sum", algo=READ, mode="contig", **kw):
    return dict(coll=coll, counts=[int(c) for c in counts], dtype=dtype, op=op, algo=algo, mode=mode, **kw)


def _check_results(r, results, cases):
    assert len(results) == len(cases)
    for res in results:
        c = res["case"]
        assert res["rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
        assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
        assert res["async"] == 0 and res["destroy_op"] == 0
        assert res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0 and res["window_calls"] == 0, (r, c, res)
        if "expect_algo" in c:
            want = c["expect_algo"]
        else:
            dev_bufs = all(m == "device" for k in ("mem", "one_mem") for m in np.atleast_1d(c.get(k, "device")))
            want = 2 if dev_bufs and c["algo"] in (READ, AUTO) else 0
        assert res["algos"] == [want] * c.get("calls", 1), f"rank {r} case {c}: ran schedules {res['algos']}"


def _run(n, cases, env=None, timeout=240, target=HW.vh_rank):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(target, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] in (0, (0, 0))
        _check_results(r, out[r]["results"], cases)
    return out


# 1. the matrix ------------------------------------------------------------------------------------
FOLDS = [("f32", "sum", {}), ("bf16", "sum", {}), ("f16", "prod", {}), ("i32", "prod", {}),
         ("f64", "max", {"special": True}), ("e4m3", "sum", {}),
         ("f32", "premul", {"s": 0.3}), ("bf16", "premul", {"s": -2.5})]


@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_matrix(dev, algo):
    """n = 3, blocks of 2051, 0 and 777 elements (several 1 KiB slices with a short last one; an empty
    block; f32: 3108 bytes, bf16: 1554 bytes -- a multiple of 2 only), contiguous and reversed with
    gaps, in and out of place: every fold of the issue's list against its reference, and the gather at
    every element size.  i32 prod wraps (full-range inputs); f64 max runs on the special values."""
    counts = [2051, 0, 777]
    cases = []
    for i, (dt, op, kw) in enumerate(FOLDS):
        cases.append(_case("rsv", counts, dt, op, algo, ("contig", "gaps")[i % 2], inplace=i % 3 == 2, seed=11 + i, **kw))
    for i, dt in enumerate(("f32", "bf16", "f64", "e4m3")):
        cases.append(_case("agv", counts, dt, "sum", algo, ("gaps", "contig")[i % 2], inplace=i % 2 == 1, seed=31 + i))
    _run(3, cases, env=SMALL)


# 2. rank counts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_rank_counts_and_block_ladder(dev, n):
    """Every rung of the fold's peer-group ladder and the path past 8 ranks, with blocks of 0, 1,
    slice - 1, slice, slice + 1 and 3 * slice + 5 elements spread over the ranks (rotated from case to
    case, so that every length meets every rank position at n = 2 too): f32 (256-element slices) and
    bf16 (512-element slices), fold and gather."""
    cases = []
    for i, (dt, coll) in enumerate((dt, coll) for dt in ("f32", "bf16") for coll in ("rsv", "agv")):
        sl = 1024 // ESZ[dt]
        ladder = [0, 1, sl - 1, sl, sl + 1, 3 * sl + 5]
        for shift in (0, 2, 4) if n < 6 else (i,):
            counts = [ladder[(q + shift + i) % 6] for q in range(n)]
            cases.append(_case(coll, counts, dt, "sum", READ, ("contig", "gaps")[(i + shift) % 2], seed=40 + 7 * i + shift,
                               null_one=True))
    _run(n, cases, env=SMALL)


# 3. mixed alignment -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16", "e4m3"])
def test_mixed_alignment_in_one_call(dev, dtype):
    """n = 3: rank 1's displacement and count are odd, so its block's byte offset and length are no
    multiples of 4 and it takes the element path, while ranks 0 and 2 (offsets and lengths multiples
    of 4 bytes) take 16-byte vectors -- in ONE call, on the read schedule; the forced ring beside it.
    The bits are the reference's on every rank."""
    q = 4 // ESZ[dtype]                     # elements per dword
    counts = [1004 * q // 2, 1003, 2050 * q]
    displs = [0, counts[0] + 1, (counts[0] + 1 + 1003 + q) // q * q + 2 * q]
    assert counts[0] * ESZ[dtype] % 4 == 0 and displs[2] * ESZ[dtype] % 4 == 0 and displs[1] % 2 == 1
    cases = []
    for i, algo in enumerate((READ, RING)):
        cases.append(_case("rsv", counts, dtype, "sum", algo, displs=displs, slack=3, seed=60 + i, calls=2))
        cases.append(_case("agv", counts, dtype, "sum", algo, displs=displs, slack=3, seed=62 + i))
        cases.append(_case("rsv", counts, dtype, "max", algo, displs=displs, inplace=True, seed=64 + i))
    _run(3, cases, env=SMALL)


# 4./5. in place, back to back, and the uniform halves ----------------------------------------------
@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
@pytest.mark.parametrize("dtype,counts,mode", [("f32", [3001, 5, 0, 700], "gaps"), ("f32", [4099] * 4, "contig"),
                                               ("bf16", [1003] * 4, "contig")],
                         ids=["uneven", "uniform-f32", "uniform-bf16"])
def test_in_place_pair_and_uniform_agreement(dev, algo, dtype, counts, mode):
    """mncclReduceScatterv in place followed by mncclAllGatherv in place with the same arrays: every
    block is then its fold on every rank and the gaps are what they were.  With uniform contiguous
    counts the fold's bits are ncclReduceScatter's, the gather's ncclAllGather's and the composition's
    ncclAllReduce's, from the same inputs."""
    n, port = 4, GW.free_port()
    e = dict(ENV, **SMALL)
    out = GW.run_ranks(HW.pair_rank, n, lambda r: (r, n, port, e, algo, dtype, counts, mode, 2), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        uniform = mode == "contig"
        assert o["rcs"] == [[0] * (5 if uniform else 2)] * 2 and o["destroy"] == 0 and o["async"] == 0, (r, o)
        assert o["bad_mid"] == [0, 0] and o["bad"] == [0, 0], (r, o)
        assert o["bad_uniform"] == ([0, 0] if uniform else []), (r, o)
        assert o["algos"] == [(algo, algo)] * 2, (r, o["algos"])
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 6. idle ranks ------------------------------------------------------------------------------------
def test_idle_ranks_and_an_all_zero_call(dev):
    """Every count 0 with every data pointer NULL: ncclSuccess, nothing launched (last_algo still -1).
    Then ranks whose own block is empty pass NULL for their one-block buffer and still take part: every
    rank -- the idle ones too -- runs the read schedule."""
    n = 4
    zero = dict(null_all=True, expect_algo=-1)
    cases = [_case("agv", [0] * n, "f32", algo=READ, seed=70, **zero),
             _case("rsv", [0] * n, "bf16", algo=READ, seed=71, **zero),
             _case("rsv", [1500, 0, 0, 333], "f32", algo=READ, mode="gaps", null_one=True, seed=72, calls=2),
             _case("agv", [0, 1500, 333, 0], "bf16", algo=AUTO, null_one=True, seed=73, calls=2),
             _case("agv", [0, 0, 777, 0], "f32", algo=RING, null_one=True, seed=74)]
    _run(n, cases, env=SMALL)


# 7. host buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [pytest.param("pinned", id="pinned"), pytest.param("pageable", id="pageable"),
                                 pytest.param(["device", "pinned", "pageable"], id="mixed")])
def test_host_buffers_run_the_padded_ring(dev, mem):
    """Pinned and pageable host memory, a placement per rank, and the two sides placed differently:
    under auto the padded ring on every rank, exact, two calls per case."""
    counts = [2051, 0, 777]
    cases = [_case("rsv", counts, "f32", "sum", AUTO, "gaps", mem=mem, expect_algo=0, seed=80, calls=2),
             _case("agv", counts, "bf16", "sum", AUTO, mem=mem, expect_algo=0, seed=81, calls=2),
             _case("rsv", counts, "bf16", "sum", AUTO, mem="device", one_mem=mem, expect_algo=0, seed=82),
             _case("agv", counts, "f32", "sum", AUTO, "gaps", mem=mem, one_mem="device", expect_algo=0, seed=83),
             _case("rsv", counts, "f32", "premul", AUTO, mem=mem, inplace=True, s=0.3, expect_algo=0, seed=84)]
    _run(3, cases, env=SMALL)


# 8. graphs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", ["rsv", "agv"])
@pytest.mark.parametrize("algo", [pytest.param(READ, id="read"), pytest.param(RING, id="ring")])
def test_graph_capture(dev, algo, coll):
    """A read-schedule call captured and replayed 3 times with fresh inputs, exact (the counts are baked
    into the graph); a forced-ring call under capture is ncclInvalidUsage on every rank and the
    communicator stays usable (the eager call after it is exact)."""
    n, port = 3, GW.free_port()
    e = dict(ENV, **SMALL)
    out = GW.run_ranks(HW.graph_rank, n, lambda r: (r, n, port, e, algo, coll, [2051, 300, 0], 3), 240, barrier=True)
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


# 9. cached consumer -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_pushes_visible_to_a_plain_load_consumer(dev, n):
    port = GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING="0")
    per = (256 << 10) // 4 // n  # about 256 KiB in all, unevenly split
    counts = [per + (q % 3) * (per // 2) + q for q in range(n)]
    out = GW.run_ranks(HW.consumer_rank, n, lambda r: (r, n, port, e, counts, 4), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0] * 4 and o["bad"] == [0] * 4, (r, o)
        assert o["algos"] == [2] * 4 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 10. refused calls --------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("local", [4] * 12), ("entry", [5, 5]), ("count", [5, 5]), ("kinds", [5]),
                                           ("uniform", [5]), ("op", [5])])
def test_refused_calls(dev, scenario, want):
    """ncclInvalidArgument (4) for check 4's local cases; ncclInvalidUsage (5) on both ranks when one
    rank passes a different array entry, calls the other collective (the other v form, or the uniform
    half) or another op -- without a hang, with nothing written, mncclCommGetAsyncError 0, and the
    communicator's next valid calls of both kinds exact."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(HW.refused_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["touched"] == 0, (r, scenario, o)
        assert o["async_after"] == 0 and o["next_rc"] == [0, 0] and o["next_bad"] == 0, (r, scenario, o)
        assert o["last_algo"] == 2 and o["async"] == 0 and o["destroy"] == 0, (r, o)
        assert o["ipc_open_failures"] == 0 and o["read_map_failures"] == 0


# 11. other contexts -------------------------------------------------------------------------------
CONTEXT_CASES = [_case("rsv", [2051, 300, 777, 5], "f32", "sum", READ, "gaps", seed=90),
                 _case("agv", [2051, 300, 777, 5], "bf16", "sum", READ, "gaps", seed=91),
                 _case("rsv", [300, 2051, 5, 777], "bf16", "premul", RING, s=0.3, inplace=True, seed=92),
                 _case("agv", [300, 2051, 5, 777], "f32", "sum", RING, inplace=True, seed=93)]


def test_one_rank(dev):
    """nranks == 1: one device copy between the block and the one-block buffer (none in place),
    whatever the schedule setting; a pre-multiplied sum scales every element, as ncclReduceScatter at
    one rank; an empty block launches nothing."""
    cases = [_case("rsv", [4099], "f32", "sum", READ, "gaps", seed=95, expect_algo=-1),
             _case("agv", [4099], "bf16", "sum", RING, "gaps", seed=96, expect_algo=-1),
             _case("rsv", [4099], "f32", "max", RING, "gaps", inplace=True, seed=97, expect_algo=-1),
             _case("rsv", [4099], "f32", "premul", READ, "gaps", s=0.3, seed=98, expect_algo=-1),
             _case("rsv", [1003], "bf16", "premul", READ, s=-2.5, inplace=True, seed=99, expect_algo=-1),
             _case("agv", [0], "f32", "sum", READ, null_all=True, seed=100, expect_algo=-1)]
    _run(1, cases)


def test_child_of_comm_split(dev):
    """Two children of two ranks each, made by ncclCommSplit from a communicator of four, run the calls
    at the same time (the cases' first two counts)."""
    cases = [dict(c, expect_algo=c["algo"]) for c in CONTEXT_CASES]
    out = _run(4, cases, env=SMALL, target=HW.split_rank)
    assert [out[r]["child"] for r in range(4)] == [(2, 0), (2, 0), (2, 1), (2, 1)]


def test_ranks_as_threads(dev):
    n, port = 4, GW.free_port()
    e = dict(ENV, **SMALL)
    out = GW.run_ranks(HW.threads_proc, 1, lambda r: (n, port, CONTEXT_CASES, e), 240)
    assert sorted(out) == [0] and "error" not in out[0], out
    for r, o in enumerate(out[0]["ranks"]):
        assert o is not None and "error" not in o, (r, o)
        assert o["destroy"] == 0
        _check_results(r, o["results"], CONTEXT_CASES)


def test_non_blocking_mode(dev):
    _run(4, [dict(c, calls=2) for c in CONTEXT_CASES], env=dict(SMALL, MINI_NCCL_BLOCKING="0"))
