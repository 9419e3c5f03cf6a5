"""ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd on the GPU (-m gpu): the HIP path through the C
ABI against the bytes themselves.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box / under MNCCL_TEST_COLOCATE=1
(gpu_workers.rank_device).  Every message is seeded random bytes (p2p_workers.msg), different per
step, pair and tag; after every step each recv holds exactly its message, each send is unchanged, and
the 256 guard bytes past every recv and every send are unchanged.  mncclCommGetAsyncError is 0 after
every step and last_algo reports the ring (0) after every point-to-point launch.
"""
import os

import pytest

import gpu_workers as GW
import p2p_workers as PW
from p2p_workers import op

pytestmark = pytest.mark.gpu

ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}
# 1 KiB slots on 2 pipelines (p2p_pipes: the budget over 2 (n - 1) pairs is far above 2, so C clamps it)
SMALL = {"MINI_NCCL_CHANNELS": "2", "MINI_NCCL_SLICE_SIZE": "1024"}
SLOTS, PIPES, SLOT = 2, 2, 1024  # MINI_NCCL_SLOTS' default
WRAP = (3 * SLOTS * PIPES * SLOT + 20) // 4   # f32 elements: the credits go round three times, a short last slice
EXACT = SLOTS * PIPES * SLOT // 4             # exactly the pair's slots
NDEV = [1]


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    NDEV[0] = out[0]["count"]
    return NDEV[0]


def _launch(*ops, group=None):
    return {"ops": list(ops)} if group is None else {"ops": list(ops), "group": group}


def _run(n, steps, env=None, timeout=180, want_rcs=None):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    steps = [dict(s, seed=s.get("seed", 100 + i)) for i, s in enumerate(steps)]
    out = GW.run_ranks(PW.p2p_rank, n, lambda r: (r, n, port, steps, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    colo = GW.colocated(dict(os.environ, **e))
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        assert out[r]["info"]["device"] == GW.rank_device(r, NDEV[0], colo), (r, out[r]["info"]["device"])
        assert len(out[r]["results"]) == len(steps)
        ran = False
        for i, res in enumerate(out[r]["results"]):
            assert all(rc == 0 for rcs in res["rcs"] for rc in rcs), f"rank {r} step {i}: result codes {res['rcs']}"
            assert res["bad"] == 0, f"rank {r} step {i}: {res['bad']} bytes differ (payload, send or guards)"
            assert res["async"] == 0, (r, i, res)
            ran = ran or not res["idle"]
            if not steps[i].get("ar") and ran:
                assert res["last_algo"] == 0, (r, i, res)  # the ring's scratch protocol
    return out


# 1. the matrix ------------------------------------------------------------------------------------
def _both_ways(dtype, count, soff=0, roff=0):
    """Ungrouped: rank 0 sends then receives, rank 1 receives then sends."""
    s, r = (lambda p, t: op("send", p, dtype, count, t, soff)), (lambda p, t: op("recv", p, dtype, count, t, roff))
    return {"launches": {0: [_launch(s(1, 0)), _launch(r(1, 1))], 1: [_launch(r(0, 0)), _launch(s(0, 1))]}}


def test_matrix_ungrouped_both_directions(dev):
    """n = 2, ungrouped, both directions: five datatypes x counts 1, 2, 4099 (shorter than a vector; a
    vector body plus an element tail); f16 / bf16 at 1001 and 1003 (bytes no multiple of 4); f16 at
    4100 with a 2-byte offset on the sender only, on the receiver only, and on both -- the ends pick
    their 16-byte or element path independently.  last_algo == 0."""
    steps = [_both_ways(dt, c) for dt in ("f32", "f64", "i32", "f16", "bf16") for c in (1, 2, 4099)]
    steps += [_both_ways(dt, c) for dt in ("f16", "bf16") for c in (1001, 1003)]
    steps += [_both_ways("f16", 4100, so, ro) for so, ro in ((2, 0), (0, 2), (2, 2))]
    _run(2, steps)


# 2. slot wrap -------------------------------------------------------------------------------------
def _ring_shift(n, count, dtype="f32", order=("send", "recv")):
    def launch(r):
        ops = {"send": op("send", (r + 1) % n, dtype, count), "recv": op("recv", (r - 1) % n, dtype, count)}
        return _launch(*(ops[k] for k in order))
    return {"launches": {r: [launch(r)] for r in range(n)}}


def test_slot_wrap(dev):
    """n = 3, 2 pipelines, 1 KiB slots: every rank runs group{send -> r + 1, recv <- r - 1} with
    3 x slots x pipes x 1024 + 20 bytes -- the credits go round three times and the last slice is
    short -- then the same at exactly slots x pipes x 1024 bytes."""
    _run(3, [_ring_shift(3, WRAP), _ring_shift(3, EXACT), _ring_shift(3, WRAP, order=("recv", "send"))], env=SMALL)


# 3. asymmetric grouping ---------------------------------------------------------------------------
def test_asymmetric_grouping(dev):
    """n = 2 at the size of the slot-wrap test: rank 0 groups its send and recv, rank 1 calls recv
    then send ungrouped; then rank 1 send then recv against rank 0's group in the other order.  Only
    waves that serve one pair each get through this once the message outgrows the slots."""
    s, r = (lambda p: op("send", p, "f32", WRAP)), (lambda p: op("recv", p, "f32", WRAP))
    steps = [{"launches": {0: [_launch(s(1), r(1))], 1: [_launch(r(0)), _launch(s(0))]}},
             {"launches": {0: [_launch(r(1), s(1))], 1: [_launch(s(0)), _launch(r(0))]}}]
    _run(2, steps, env=SMALL)


# 4. all pairs -------------------------------------------------------------------------------------
def _all_pairs(n, ranks, shift=0):
    """One group per rank of `ranks`: a send to and a recv from every rank of `ranks`, itself
    included.  The count differs per pair and is 0 for some; the datatype alternates per pair."""
    counts = (4099, 0, 1003, 70001, 2, 300, 1)
    cnt = lambda a, b: counts[(3 * a + 2 * b + shift) % len(counts)]
    dt = lambda a, b: ("f32", "f16")[(a + b) % 2]
    return {"launches": {r: [_launch(*([op("send", q, dt(r, q), cnt(r, q)) for q in ranks] +
                                       [op("recv", q, dt(q, r), cnt(q, r)) for q in ranks]), group=True)]
                         for r in ranks}}


def test_all_pairs(dev):
    """n = 4: one group of 3 sends + 3 recvs + the self pair per rank, counts differing per pair and
    including 0, f32 and f16 mixed per pair: the permutation byte for byte.  Then rank 3 idle: it makes
    no call at all while ranks 0-2 exchange."""
    n = 4
    full = _all_pairs(n, range(n))
    assert any(o["count"] == 0 for o in full["launches"][0][0]["ops"] + full["launches"][1][0]["ops"])
    out = _run(n, [full, _all_pairs(n, range(3), shift=1), _all_pairs(n, range(n), shift=2)])
    assert [res["idle"] for res in out[3]["results"]] == [False, True, False]


# 5. order -----------------------------------------------------------------------------------------
def test_order_within_a_pair(dev):
    """Two sends of different sizes to one peer in one group, received by two ungrouped recvs, and the
    reverse: two ungrouped sends received by one group of two recvs.  Call order per pair."""
    big, small = op("send", 1, "f32", WRAP, tag=0), op("send", 1, "f16", 1003, tag=1)
    rbig, rsmall = op("recv", 0, "f32", WRAP, tag=0), op("recv", 0, "f16", 1003, tag=1)
    steps = [{"launches": {0: [_launch(big, small)], 1: [_launch(rbig), _launch(rsmall)]}},
             {"launches": {0: [_launch(small, big)], 1: [_launch(rsmall), _launch(rbig)]}},
             {"launches": {0: [_launch(big), _launch(small)], 1: [_launch(rbig, rsmall)]}}]
    _run(2, steps, env=SMALL)


# 6. interleaving ----------------------------------------------------------------------------------
def test_interleaved_with_allreduces(dev):
    """n = 3, four steps in a row on one communicator: a p2p ring shift, ncclAllReduce forced to the
    ring, ncclAllReduce with the default schedule, the p2p ring shift again -- all bit-exact (the
    all-reduces against the oracle), async == 0: the counters every schedule shares stay in step."""
    n = 3
    steps = [_ring_shift(n, 70001), {"ar": True, "algo": 0, "count": 3 * 4099 + 1},
             {"ar": True, "algo": -1, "count": 3 * 70001 + 2}, _ring_shift(n, 70001, "f16")]
    out = _run(n, steps)
    for r in range(n):
        assert [res["last_algo"] for res in out[r]["results"]][:2] == [0, 0], out[r]["results"]


# 7. graphs ----------------------------------------------------------------------------------------
def test_graph_capture(dev):
    """n = 2: a grouped exchange captured once and replayed three times, with new send contents before
    each replay (no host rendezvous, counters on the device: the replays stay in step), then an eager
    exchange on the same communicator."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(PW.graph_rank, n, lambda r: (r, n, port, ENV, 70001, 3), 180, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["capture_rc"] == [0, 0, 0] and o["captured_algo"] == 0 and o["bad"] == [0, 0, 0], (r, o)
        assert o["eager_rc"] == [0, 0, 0] and o["eager_bad"] == 0, (r, o)
        assert o["async"] == 0 and o["destroy"] == 0 and o["last_algo"] == 0, (r, o)


# 8. threads and one rank --------------------------------------------------------------------------
def test_ranks_as_threads(dev):
    """Three ranks as threads of one process, one group each: what thread_local group state buys."""
    n, port = 3, GW.free_port()
    out = GW.run_ranks(PW.threaded_ranks_proc, 1, lambda r: (n, port, ENV, 20011), 180)
    assert sorted(out) == [0] and "error" not in out[0], out
    ranks = out[0]["ranks"]
    assert sorted(ranks) == list(range(n)), ranks
    for r in range(n):
        o = ranks[r]
        assert "error" not in o, o.get("error")
        assert [x["rcs"] for x in o["results"]] == [[0, 0, 0]] * 2 and [x["bad"] for x in o["results"]] == [0, 0], (r, o)
        assert o["async"] == 0 and o["destroy"] == 0 and o["last_algo"] == 0, (r, o)


def test_one_rank(dev):
    """nranks == 1: the self pair copies (f16 from a 2-byte offset, f32 over several waves); alone, a
    send to rank 0 is ncclInvalidUsage (5) ungrouped and at ncclGroupEnd; a pair of different sizes is
    ncclInvalidUsage at ncclGroupEnd with nothing written; the communicator then still copies."""
    port = GW.free_port()
    out = GW.run_ranks(PW.one_rank, 1, lambda r: (port, ENV), 120)
    assert sorted(out) == [0], out
    o = out[0]
    assert "error" not in o, o.get("error")
    assert o["rcs"] == [[0, 0, 0], [0, 0, 0], [5], [0, 5], [0, 0, 5], [0, 0, 0]], o
    assert o["bad"] == [0] * 6, o
    assert o["async"] == 0 and o["destroy"] == 0 and o["last_algo"] == 0, o


# 9. errors on a live communicator -----------------------------------------------------------------
@pytest.mark.parametrize("scenario,want", [("peer_range", [4, 4]), ("self", [5, 5]), ("overlap", [0, 4, 0, 4]),
                                           ("stream", [0, 5, 5]), ("pageable", [4, 4]), ("pinned", [0, 0, 0]),
                                           ("too_many", [0, 0, 0, 5, 5])])
def test_errors_on_a_live_communicator(dev, scenario, want):
    """Each refusal (4 ncclInvalidArgument, 5 ncclInvalidUsage) launches nothing, leaves
    mncclCommGetAsyncError at 0, and is followed by a correct grouped exchange: the communicator
    survived.  Pinned host buffers succeed."""
    n, port = 2, GW.free_port()
    out = GW.run_ranks(PW.errors_rank, n, lambda r: (r, n, port, ENV, scenario), 120, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == want, (r, scenario, o)
        assert o["touched"] == 0 and o["async_after"] == 0, (r, scenario, o)
        assert o["next_rc"] == [0, 0, 0] and o["bad"] == 0, (r, scenario, o)
        assert o["async"] == 0 and o["destroy"] == 0 and o["last_algo"] == 0, (r, scenario, o)
