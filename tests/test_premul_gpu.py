"""Pre-multiplied sums (ncclRedOpCreatePreMulSum / ncclRedOpDestroy) on the GPU (-m gpu): the HIP
path through the C ABI against the oracle's ncclSum on inputs scaled in numpy, bit for bit
(tests/premul_ref.py; NaN payloads excepted, as for every arithmetic op).

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box (gpu_workers.rank_device).
Every call of every case is checked, 256 guard bytes past each recv included.
"""
import pytest

import boundary_cases as BC
import gpu_workers as GW
import premul_ref as P
import premul_workers as PW

pytestmark = pytest.mark.gpu

RING, READ, ONESHOT, GRID, AUTO = 0, 2, 3, 4, -1
ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    return out[0]["count"]


def _run(n, cases, env=None, timeout=240):
    port = GW.free_port()
    e = dict(ENV, **(env or {}))
    out = GW.run_ranks(PW.premul_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        assert len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0 and res["destroy_rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']} / {res['destroy_rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
            assert res["async"] == 0
            want = c.get("expect_algo", c["algo"])
            assert res["algo"] == want, f"rank {r} case {c}: ran schedule {res['algo']}"
            assert res["grid"] == c.get("expect_grid", 0), f"rank {r} case {c}: {res['grid']} grid calls"
    return out


# 1. parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_parity_with_sum_of_scaled_inputs(dev, n):
    """ncclAllReduce / ncclReduceScatter / ncclReduce, forced ring and forced read, in place and out of
    place, on one pipeline: chunks of 4099 elements with an all-reduce tail of n - 1, and chunks whose
    last slice is two full fold batches, 5 vectors and one element (premul_ref.parity_cases); all five
    datatypes at 3 ranks, f32 and bf16 at 2 / 5 / 8, f32 at 9 (the one-peer-ahead fold)."""
    _run(n, P.parity_cases(n), env=BC.ONE, timeout=300)


def test_parity_with_the_smallest_slices(dev):
    """16-byte slices on 4 pipelines over 2 slots: a chunk spans 13 or 25 slices and the ring's slots
    wrap; bf16's last slice is 8 bytes, the element path."""
    _run(3, P.tiny_slice_cases(3), env=P.TINY)


# 2. one rank --------------------------------------------------------------------------------------
def test_one_rank_scales_every_element(dev):
    """nranks == 1 is no copy: recv = round(s * send) over all `count` elements -- the scale kernel --
    through all three collectives, counts 1 and 4099, in place and out of place, every datatype."""
    cases = []
    for dt in P.DTYPES:
        for count in (1, 4099):
            for inplace in (False, True):
                k = len(cases)
                choice = [s for s in P.scalars(dt, 1) if s != 1.0]  # (1 / n is 1 here: it would be a copy)
                cases.append(dict(dtype=dt, s=choice[k % len(choice)], count=count, inplace=inplace, seed=P.SEED + 600 + k))
    port = GW.free_port()
    out = GW.run_ranks(PW.one_rank, 1, lambda r: (cases, ENV, port), 120)
    assert 0 in out and "error" not in out[0], out
    assert out[0]["destroy"] == 0 and len(out[0]["results"]) == len(cases)
    for res in out[0]["results"]:
        assert all(rc == 0 for rc in res["rcs"]) and res["bad"] == 0, res
        assert res["algo"] == -1, res  # no collective kernel ran


# 3. auto ------------------------------------------------------------------------------------------
def test_auto_grid_form_and_one_shot_routing(dev):
    """Two ranks under auto.  4 MiB chunks of device memory: the grid form scales inside its fold
    (read_grid_calls counts the call, last_algo reports the read schedule).  A 16 KiB call on pinned
    host buffers: ncclSum runs one-shot; a pre-multiplied sum has no one-shot form and, as the header
    documents, runs as a call the one-shot does not fit -- the ring here, since host buffers cannot
    take the read schedule.  A forced one-shot behaves the same way; on device buffers it is the
    read schedule's persistent kernel."""
    big = (4 << 20) // 4
    cases = [
        dict(coll="ar", dtype="f32", s=0.5, chunk=big, tail=1, algo=AUTO, expect_algo=READ, expect_grid=1, seed=P.SEED + 700),
        dict(coll="ar", dtype="bf16", s=0.3, chunk=2 * big, tail=0, inplace=True, algo=AUTO, expect_algo=READ, expect_grid=1,
             seed=P.SEED + 701),
        dict(coll="ar", dtype="f32", s=0.3, chunk=big, tail=0, algo=GRID, expect_algo=READ, expect_grid=1, seed=P.SEED + 702),
        dict(coll="ar", dtype="f32", s=None, chunk=2048, tail=3, algo=AUTO, mem="pinned", expect_algo=ONESHOT, seed=P.SEED + 703),
        dict(coll="ar", dtype="f32", s=0.3, chunk=2048, tail=3, algo=AUTO, mem="pinned", expect_algo=RING, seed=P.SEED + 704),
        dict(coll="ar", dtype="f32", s=-2.5, chunk=2048, tail=3, algo=ONESHOT, mem="pinned", expect_algo=RING, seed=P.SEED + 705),
        dict(coll="ar", dtype="f32", s=-2.5, chunk=2048, tail=3, algo=ONESHOT, expect_algo=READ, seed=P.SEED + 706),
        dict(coll="ar", dtype="f32", s=None, chunk=2048, tail=3, algo=ONESHOT, expect_algo=ONESHOT, seed=P.SEED + 707),
    ]
    _run(2, cases)


@pytest.mark.parametrize("n", [3, 4, 5, 8])
def test_grid_form_at_every_peer_group(dev, n):
    """The grid kernel's other instantiations -- G = 2 and 4 peer slots with one vector per lane, 4 and
    7 with two (boundary_cases.grid_rule_v) -- forced, with the smallest MINI_NCCL_GRID_MIN: chunks of
    64 KiB and one more vector (a last workgroup of 16 bytes) and of whole workgroups, all five
    datatypes, an all-reduce tail of n - 1 on every other call."""
    cases = []
    for dt in P.DTYPES:
        ss = P.scalars(dt, n)
        for rem in (16, 0):
            k = len(cases)
            cases.append(dict(coll="ar", dtype=dt, s=ss[k % len(ss)], chunk=(BC.GRID_FLOOR + rem) // BC.ESZ[dt],
                              tail=(n - 1) * (k % 2), inplace=k % 3 == 1, algo=GRID, expect_algo=READ, expect_grid=1,
                              seed=P.SEED + 800 + k))
    _run(n, cases, env=BC.grid_env(n))


# 4. registered windows ----------------------------------------------------------------------------
WIN = {"MINI_NCCL_TIMEOUT_MS": "20000", "MINI_NCCL_WINDOW_RENDEZVOUS": "0"}


def test_registered_windows_parity(dev):
    n, port = 3, GW.free_port()
    out = GW.run_ranks(PW.window_rank, n, lambda r: (r, n, port, WIN, "parity"), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rcs"] == [0, 0, 0] and o["bad"] == [0, 0, 0], (r, o)
        assert o["wc"] == [1, 1, 1] and o["algos"] == [READ] * 3, (r, o)  # launched without a rendezvous
        assert o["info"]["window_fast"] == 1 and o["destroy"] == 0


def test_registered_windows_scalar_mismatch_is_invalid_usage(dev):
    import mini_nccl as M
    n, port = 3, GW.free_port()
    out = GW.run_ranks(PW.window_rank, n, lambda r: (r, n, port, WIN, "mismatch"), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        assert "error" not in out[r], out[r].get("error")
        assert out[r]["rc"] == M.ncclInvalidUsage, (r, out[r])


# 5. negotiated mismatch ---------------------------------------------------------------------------
def test_negotiated_scalar_mismatch(dev):
    import mini_nccl as M
    n, port = 2, GW.free_port()
    out = GW.run_ranks(PW.mismatch_rank, n, lambda r: (r, n, port, ENV), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["rc"] == M.ncclInvalidUsage and o["rc_reduce"] == M.ncclInvalidUsage, (r, o)
        assert o["written"] == 0 and o["written_reduce"] == 0 and o["async_after"] == 0, (r, o)
        assert o["next"] == (0, 0), (r, o)                  # a correct call afterwards
        assert o["swapped"] == [(0, 0), (0, 0)], (r, o)     # equal scalars, handles in another order
        assert o["info"]["last_algo"] == READ and o["destroy"] == 0
    assert out[0]["handles"] != out[1]["handles"]          # the handle numbers did differ


# 6. handles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocking", ["1", "0"])
def test_handles(dev, blocking):
    import mini_nccl as M
    n, port = 2, GW.free_port()
    e = dict(ENV, MINI_NCCL_BLOCKING=blocking)
    out = GW.run_ranks(PW.handles_rank, n, lambda r: (r, n, port, e), 240, barrier=True)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["blocking"] == int(blocking)
        assert o["create_rcs"] == [0] * 16 + [M.ncclInvalidUsage], (r, o)       # 16 live, the 17th refused
        assert o["handles"] == list(range(M.MNCCL_FIRST_USER_OP, M.MNCCL_FIRST_USER_OP + 16)), (r, o)
        assert o["destroy_mid"] == 0 and o["recreate"] == (0, o["handles"][7]), (r, o)  # the slot again
        assert o["full_again"] == M.ncclInvalidUsage and o["recreated_call"] == (0, 0), (r, o)
        assert o["destroy_all"] == [0] * 16, (r, o)
        assert o["wrong_dtype"] == [M.ncclInvalidArgument] * 3, (r, o)
        assert o["unknown"] == [M.ncclInternalError] * 3, (r, o)
        assert o["destroy_builtin"] == [M.ncclInvalidArgument] * 4, (r, o)
        assert o["device_residence"] == M.ncclInvalidUsage and o["bad_dtype"] == M.ncclInternalError, (r, o)
        assert o["local_reduce"] == M.ncclInternalError and o["avg"] == M.ncclInternalError, (r, o)
        assert o["early_destroy"] == (0, 0, 0, True), (r, o)  # destroyed (and its slot reused) once issued
        assert o["usable"] == [(0, 0)] * 5, (r, o)            # usable after every refusal
        assert o["async"] == 0 and o["destroy"] == 0


# 7. graph -----------------------------------------------------------------------------------------
def test_graph_replays_after_the_op_is_destroyed(dev):
    n, port = 2, GW.free_port()
    out = GW.run_ranks(PW.graph_rank, n, lambda r: (r, n, port, ENV, 3), 240)
    assert sorted(out) == list(range(n)), out
    for r in range(n):
        o = out[r]
        assert "error" not in o, o.get("error")
        assert o["capture_rc"] == [0] and o["destroy_rc"] == 0 and o["reused"], (r, o)
        assert o["captured_algo"] == READ and o["bad"] == [0, 0, 0] and o["async"] == 0, (r, o)
