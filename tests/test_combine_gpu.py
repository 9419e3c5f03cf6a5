"""mncclAllToAllvCombine on the GPU (-m gpu) against the rule restated in numpy, bit for bit
(combine_workers.Shape.expect); the elements between rows and the guard bytes stay unchanged."""
import numpy as np
import pytest

import combine_workers as CW
import gpu_workers as GW
from test_alltoallv_gpu import ENV, READ, RING, SMALL, _pattern, dev  # noqa: F401 (dev: the device fixture)

pytestmark = pytest.mark.gpu


def _run(n, cases, env=None):
    port, e = GW.free_port(), dict(ENV, **(env or {}))
    out = GW.run_ranks(CW.combine_rank, n, lambda r: (r, n, port, cases, e), 240, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        for res in out[r]["results"]:
            c = res["case"]
            want = c.get("want_rc", 0)
            assert res["rcs"] == [want], f"rank {r} case {c}: ncclResult {res['rcs']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} bytes differ"
            assert res["async"] == 0 and res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0, (r, c, res)
            if want == 0 and "expect_algo" in c:
                assert res["algos"] == [c["expect_algo"]] * (2 if c.get("graph") else 1), (r, c, res["algos"])


@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_matrix(dev, algo, dtype):
    """n = 3, counts from {0, 1, 3, 70} rows, rows of 1, 7, 64, 257 and 1031 elements at stride rowcount and
    rowcount + 5, topk 1, 3 and 9 (past the group of 8), weights given and NULL, nrows 70 / 0 / 33 by rank,
    slots of every invalid kind.  The weighted f32 cases with topk > 1 have seeds 23, 26, 39 and 42: with them
    a fused multiply-add gives other bits than the rule's separate product and sum in 254, 2600, 4733 and
    22529 elements (counted once on the CPU with a float64 emulation of the fused form)."""
    cases = [dict(C=_pattern(3, (70, 0, 1, 3), i), dtype=dtype, rowcount=rc, pad=pad, topk=(1, 3, 9)[(i + j) % 3],
                  weights=(i + j) % 2 == 0, nrows=[70, 0, 33], algo=algo, expect_algo=algo, seed=10 + 8 * i + pad)
             for i, rc in enumerate((1, 7, 64, 257, 1031)) for j, pad in enumerate((0, 5))]
    _run(3, cases)


@pytest.mark.parametrize("n", [2, 5, 8, 9])
def test_slices_cut_rows(dev, n):
    """1 KiB slices on 4 pipelines, rows of 1028 and 3000 bytes (no slice boundary falls on a row's),
    nrows 40 / 0 / 2 by rank: the ranks run out at different slices."""
    cases = [dict(C=_pattern(n, (40, 0, 2), i), dtype=dt, rowcount=rb // CW.ESZ[dt], pad=pad, topk=k, nrows=[40, 0, 2],
                  algo=READ, expect_algo=READ, seed=50 + i)
             for i, (rb, dt, pad, k) in enumerate(((1028, "f32", 0, 2), (3000, "bf16", 0, 3), (3000, "f16", 3, 9), (1028, "bf16", 0, 1)))]
    _run(n, cases, env=SMALL)


@pytest.mark.parametrize("rowcount", [257, 258])
def test_mixed_alignment(dev, rowcount):
    """bf16, rank 1's sendbuff and rank 0's recvbuff 2 bytes off: rank 0 folds element by element, rank 1
    serves an odd send that takes every puller of it off the vector path; both schedules, the same bits."""
    cases = [dict(C=_pattern(3, (3, 70, 1), 1), dtype="bf16", rowcount=rowcount, pad=pad, topk=2, nrows=[33, 70, 5], algo=algo,
                  expect_algo=algo, seed=60 + pad, send_off=[0, 2, 0], recv_off=[2, 0, 0]) for pad in (0, 1, 2) for algo in (READ, RING)]
    _run(3, cases)


@pytest.mark.parametrize("algo", [READ, RING])
def test_round_trip_with_dispatch(dev, algo):
    cases = [dict(C=_pattern(3, (70, 3, 0, 9), i), dtype=dt, rowcount=rc, topk=1, nrows=[1], algo=algo, dispatch=True, seed=70 + i)
             for i, (dt, rc) in enumerate((("bf16", 1030), ("f32", 64), ("f16", 7)))]
    _run(3, cases)


def test_graph_rereads_slots_and_weights(dev):
    """A captured read-schedule call replayed twice, slotidx and weights rewritten in between: each replay
    matches what it ran with.  On a forced ring the capture is ncclInvalidUsage everywhere; the next call is exact."""
    base = dict(C=_pattern(3, (70, 0, 3, 9)), dtype="bf16", rowcount=1030, pad=1, topk=3, nrows=[70, 0, 33])
    cases = [dict(base, algo=READ, expect_algo=READ, graph=True, seed=80),
             dict(base, dtype="f32", rowcount=24, algo=READ, expect_algo=READ, graph=True, seed=81),
             dict(base, algo=RING, graph=True, seed=82, want_rc=5),
             dict(base, algo=RING, expect_algo=RING, seed=83)]
    _run(3, cases)


@pytest.mark.parametrize("n", [3, 1])
def test_refusals_and_idle_ranks(dev, n):
    """The local refusals (every rank alike) and the ones after the rendezvous (rank 1 differs): nothing
    written, the communicator still usable.  A rank that only sends, one that only pulls, the all-zero
    call (zero-filled rows), and one rank."""
    C = np.array(_pattern(n, (70, 3, 9)))
    base = dict(C=C.tolist(), dtype="bf16", rowcount=300, pad=1, topk=2, nrows=[33, 9, 70], algo=READ)
    local = [dict(topk=0), dict(topk=17), dict(rowcount=0), dict(stride=299), dict(nrows=1 << 30), dict(send=None), dict(recv=None),
             dict(idx=None), dict(rowcount=1 << 30, stride=1 << 30), dict(rd=[2] * n), dict(recv="W"), dict(idx="HOST"), dict(w="HOST")]
    cases = [dict(base, seed=90 + i, over=o, over_all=True, want_rc=4) for i, o in enumerate(local) if n > 1 or "rd" not in o]
    cases.append(dict(base, seed=105, group=True, want_rc=5))  # an open group: refused, and the group stays clean
    only_sends = C * (np.arange(n) != n - 1)  # the last rank gets no rows back; below it also has no output rows
    only_pulls = C * (np.arange(n) != 0)[:, None]  # rank 0 sends nothing
    cases += [dict(base, seed=110, nrows=[33, 9, 0], C=only_sends.tolist()), dict(base, seed=111, C=only_pulls.tolist(), algo=RING),
              dict(base, seed=112, C=np.zeros((n, n), int).tolist()), dict(base, seed=113)]
    if n > 1:
        cases[-1:-1] = [dict(base, seed=114, over=dict(rowcount=301), want_rc=5),
                        dict(base, seed=115, over=dict(rc=[int(C[0, 1]) + 1] + [int(v) for v in C[1:, 1]]), want_rc=5)]
    _run(n, cases)


@pytest.mark.parametrize("algo", [pytest.param(READ, id="read"), pytest.param(RING, id="ring")])
def test_rank_with_neither_buffer_takes_part(dev, algo):
    """n = 2: rank 1 sends nothing, has no output rows and passes NULL for sendbuff, recvbuff, slotidx and
    weights; on the read schedule the communicator's stub stands in for its buffers in the rendezvous.
    Rank 0 folds its own two rows of 128 bf16, exact; ncclSuccess and the same schedule on both ranks."""
    case = dict(C=[[2, 0], [0, 0]], dtype="bf16", rowcount=128, topk=2, nrows=[2, 0], algo=algo, expect_algo=algo, seed=120,
                over=dict(send=None, recv=None, idx=None, w=None))
    _run(2, [case])
