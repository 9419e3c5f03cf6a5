"""The fp8 datatypes (ncclFloat8e4m3 / ncclFloat8e5m2) on the GPU (-m gpu): the HIP path through the
C ABI against tests/fp8_ref.py, byte for byte over every element; where the reference is NaN the
library's result must be a NaN of the format, and nothing else may differ.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box (gpu_workers.rank_device).
"""
import pytest

import boundary_cases as BC
import fp8_ref as F
import fp8_workers as W
import gpu_workers as GW

pytestmark = pytest.mark.gpu

RING, READ, ONESHOT, GRID, AUTO = 0, 2, 3, 4, -1
ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}


@pytest.fixture(scope="module")
def dev(nccl_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    return out[0]["count"]


# 1. every operand pair ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs(dev):
    out = GW.run_ranks(W.exhaustive_fold, 1, lambda r: (), 180)
    assert 0 in out and "error" not in out[0], out
    return out[0]["results"]


@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "element"])
@pytest.mark.parametrize("op", F.OPS)
@pytest.mark.parametrize("fmt", list(F.FORMATS))
def test_every_operand_pair(pairs, fmt, op, offset):
    """mncclLocalReduce over all 65 536 (local, incoming) pairs: the hardware conversions plus the
    clamp against the contract -- rounding, subnormals, saturation, inf, NaN, the sign of zero, and
    which operand Max / Min return.  Dword-aligned buffers run the 16-byte kernel, the same buffers
    one byte further the element kernel.  (Fails where the library has no fp8: ncclInternalError.)"""
    rc, bad, first = pairs[(fmt, op, offset)]
    assert rc == 0, f"ncclResult {rc}"
    assert bad == 0, f"{bad} mismatches; (local, incoming, got, expected): {[tuple(hex(v) for v in t) for t in first]}"


# 2. every input under every scalar ----------------------------------------------------------------
def test_every_input_under_every_scalar(dev):
    """nranks == 1 with a pre-multiplied sum is out = encode(s * x): all 256 x 256 per format, the 256
    ops created and destroyed in turn."""
    port = GW.free_port()
    out = GW.run_ranks(W.exhaustive_scale, 1, lambda r: (ENV, port), 180)
    assert 0 in out and "error" not in out[0], out
    assert out[0]["destroy"] == 0
    for fmt in F.FORMATS:
        res = out[0]["results"][fmt]
        assert res["rcs"] == [0], (fmt, res)
        assert res["bad"] == 0, f"{fmt}: {res['bad']} mismatches, first (scalar, input, got, expected) {res['first']}"
        assert res["algo"] == -1, res  # no collective kernel ran


# 3. the folding collectives -----------------------------------------------------------------------
def shape_b(n, extra):
    """A chunk whose last slice under one pipeline is two full fold batches, 5 vectors and `extra`
    bytes (premul_ref.shape_b_chunk's construction; a one-byte type folds in the 4-byte types' batches)."""
    return BC.chunk_bytes(2 * BC.fold_batch(n, 1) + 5, extra)


def parity_cases(n, fmt, ops):
    """Per op: ncclAllReduce / ncclReduceScatter / ncclReduce x forced ring / forced read x five chunk
    lengths -- 4100 (vectors, the last one short), 4099 and 4098 (the element path), two fold batches
    + 5 vectors + 1 byte (element path) and + 4 bytes (the same length on the vector path) -- with
    placement and input set ("plain": nothing saturates, nothing is NaN; "wild": all 256 codes)
    turning so that every (op, collective, schedule) meets both of each."""
    out = []
    lengths = (4100, 4099, 4098, shape_b(n, 1), shape_b(n, 4))
    for oi, op in enumerate(ops):
        for ci, coll in enumerate(("ar", "rs", "rd")):
            for ai, algo in enumerate((RING, READ)):
                for li, chunk in enumerate(lengths):
                    k = len(out)
                    out.append(dict(coll=coll, fmt=fmt, op=op, s=(0x34, 0xC1, 0x2B)[(k + oi) % 3] if op == "premul" else None,
                                    chunk=chunk, tail=(n - 1) if coll == "ar" else 0, inplace=(li + ai + ci) % 2 == 1,
                                    algo=algo, root=(n - 1) if li % 2 else 0, kind=("plain", "wild")[(li + ai + oi) % 2],
                                    seed=8000 + 1000 * oi + k))
    return out


def check_plain_cases(n, cases):
    """On the CPU, before anything runs: the reference of every "plain" case holds no NaN and
    saturated nowhere, so those cases compare every byte exactly."""
    for c in cases:
        if c["kind"] != "plain":
            continue
        stats = {}
        xs = F.inputs(n, W.case_count(c, n), c["fmt"], c["seed"], "plain")
        for r in ((c["root"],) if c["coll"] == "rd" else range(n)):
            W.expected(F, c, xs, r, stats)
        assert stats.get("sat", 0) == 0 and stats.get("nan", 0) == 0, (c, stats)


def run_folds(n, cases, env=None, timeout=300):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(W.fold_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0 and len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0 and res["destroy_rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']} / {res['destroy_rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
            assert res["async"] == 0
            assert res["algo"] == c.get("expect_algo", c["algo"]), f"rank {r} case {c}: ran schedule {res['algo']}"
            assert res["grid"] == c.get("expect_grid", 0), f"rank {r} case {c}: {res['grid']} grid calls"
    return out


ALL_OPS = F.OPS + ("premul",)


@pytest.mark.parametrize("n,fmt,ops", [(3, "e4m3", ALL_OPS), (3, "e5m2", ALL_OPS), (2, "e4m3", ("sum",)),
                                       (5, "e4m3", ("sum",)), (8, "e4m3", ("sum",))],
                         ids=["n3-e4m3", "n3-e5m2", "n2", "n5", "n8"])
def test_collectives_match_the_reference(dev, n, fmt, ops):
    """The three folding collectives on both schedules against the reference's association, one
    pipeline (boundary_cases.ONE); 256 guard bytes past every recv."""
    cases = parity_cases(n, fmt, ops)
    assert {c["kind"] for c in cases} == {"plain", "wild"} and {c["inplace"] for c in cases} == {False, True}
    check_plain_cases(n, cases)
    run_folds(n, cases, env=BC.ONE)


# 4. forms -----------------------------------------------------------------------------------------
def test_one_shot_and_host_buffers(dev):
    """A forced one-shot on a 4100-byte call (fp8_oneshot, vector and element paths), and the same
    call on pinned and pageable host buffers (which the read schedule cannot take)."""
    cases = []
    for k, (fmt, op, chunk, mem, algo, want) in enumerate((
            ("e4m3", "sum", 2050, "device", ONESHOT, ONESHOT), ("e5m2", "max", 2050, "device", ONESHOT, ONESHOT),
            ("e5m2", "prod", 2049, "device", ONESHOT, ONESHOT), ("e4m3", "sum", 2050, "pinned", AUTO, ONESHOT),
            ("e4m3", "min", 2049, "pageable", RING, RING), ("e5m2", "sum", 2050, "pinned", RING, RING))):
        cases.append(dict(coll="ar", fmt=fmt, op=op, chunk=chunk, tail=1, inplace=k % 2 == 1, algo=algo, expect_algo=want,
                          kind="wild", mem=mem, seed=8800 + k))
    run_folds(2, cases)


@pytest.mark.parametrize("n", [3, 5])
def test_grid_form(dev, n):
    """The grid form (fp8_grid: one vector per lane at 3 ranks, two at 5), auto and forced, with the
    smallest MINI_NCCL_GRID_MIN: chunks of 64 KiB and one more vector."""
    cases = []
    for k, (fmt, op, algo) in enumerate((("e4m3", "sum", AUTO), ("e5m2", "sum", GRID), ("e4m3", "premul", GRID),
                                         ("e5m2", "min", AUTO), ("e4m3", "prod", GRID))):
        cases.append(dict(coll="ar", fmt=fmt, op=op, s=0x34 if op == "premul" else None, chunk=BC.GRID_FLOOR + 16,
                          tail=(n - 1) * (k % 2), inplace=k % 3 == 1, algo=algo, expect_algo=READ, expect_grid=1,
                          kind=("wild", "plain")[k % 2], seed=8900 + k))
    check_plain_cases(n, cases)
    run_folds(n, cases, env=BC.grid_env(n))


def test_registered_windows(dev):
    n, port = 3, GW.free_port()
    env = {"MINI_NCCL_TIMEOUT_MS": "20000", "MINI_NCCL_WINDOW_RENDEZVOUS": "0"}
    out = GW.run_ranks(W.window_rank, n, lambda r: (r, n, port, env), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rc"] == 0 and o["bad"] == 0 and o["destroy"] == 0, (r, o)
        assert o["wc"] == 1 and o["algo"] == READ and o["fast"] == 1, (r, o)  # launched without a rendezvous


def test_graph_capture_and_replay(dev):
    n, port = 2, GW.free_port()
    out = GW.run_ranks(W.graph_rank, n, lambda r: (r, n, port, ENV, 2), 240)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["capture_rc"] == [0] and o["captured_algo"] == READ and o["bad"] == [0, 0] and o["async"] == 0, (r, o)


# 5. the calls that only move bytes ----------------------------------------------------------------
def test_movers(dev):
    """ncclAllGather, ncclBroadcast, ncclAllToAll, ncclGather, ncclScatter and ncclAllToAllv with
    element size 1, at 3 ranks: 4099 elements (the element path) and 4100 (vectors), ring and read."""
    n, cases = 3, []
    for coll in ("ag", "bc", "a2a", "ga", "sc", "a2av"):
        for count in (4099, 4100):
            for algo in (RING, READ):
                k = len(cases)
                cases.append(dict(coll=coll, fmt=("e4m3", "e5m2")[k % 2], count=count, algo=algo, root=k % n, seed=9000 + k))
    port = GW.free_port()
    out = GW.run_ranks(W.mover_rank, n, lambda r: (r, n, port, cases, dict(ENV, **BC.ONE)), 300, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0 and len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0 and res["async"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} bytes differ"
            assert res["algo"] == c["algo"], f"rank {r} case {c}: ran schedule {res['algo']}"


def test_send_recv_ring(dev):
    """A grouped ncclSend / ncclRecv ring with odd and even byte counts (one slice and several), once
    into a registered window -- the sender pushes direct -- and once outside it."""
    n, port = 3, GW.free_port()
    counts = (4099, 4100, 1, 1027)
    env = dict(ENV, MINI_NCCL_CHANNELS="2", MINI_NCCL_SLICE_SIZE="1024")
    out = GW.run_ranks(W.p2p_ring_rank, n, lambda r: (r, n, port, counts, env), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["destroy"] == 0 and len(o["results"]) == 2 * len(counts)
        for res in o["results"]:
            assert res["rcs"] == [0, 0, 0] and res["async"] == 0, (r, res)
            assert res["bad"] == 0, (r, res)
            assert res["direct"] == (1 if res["where"] == "win" else 0), (r, res)
