"""mncclAllToAllvRows on the GPU (-m gpu) against numpy fancy indexing, byte for byte
(rows_workers.Shape.expect); the bytes around the recv blocks and the send side must stay unchanged."""
import numpy as np
import pytest

import gpu_workers as GW
import rows_workers as RW
from test_alltoallv_gpu import ENV, READ, RING, SMALL, _pattern, dev  # noqa: F401 (dev: the device fixture)

pytestmark = pytest.mark.gpu


def _run(n, cases, env=None, want_rc=0):
    port, e = GW.free_port(), dict(ENV, **(env or {}))
    out = GW.run_ranks(RW.rows_rank, n, lambda r: (r, n, port, cases, e), 240, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        for res in out[r]["results"]:
            c = res["case"]
            want = c.get("want_rc", want_rc)
            assert res["rcs"] == [want], f"rank {r} case {c}: ncclResult {res['rcs']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} bytes differ"
            assert res["async"] == 0 and res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0, (r, c, res)
            if want == 0:
                assert res["algos"] == [c.get("expect_algo", c["algo"])] * (2 if c.get("graph") else 1), (r, c, res["algos"])


@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_matrix(dev, algo, esz):
    """n = 3, counts from {0, 1, 3, 70} rows (70 crosses the 64-index batch), rows of 1, 7, 64, 257 and
    1031 elements -- below one vector, narrow with and without a 16-byte tail, wide and no multiple of
    16 or 1024 bytes -- at stride rowcount and rowcount + 5, top-2 indices, overlapping sdispls ranges."""
    cases = [dict(C=_pattern(3, (70, 0, 1, 3), i), esz=esz, rowcount=rc, pad=pad, algo=algo, seed=10 * i + pad)
             for i, rc in enumerate((1, 7, 64, 257, 1031)) for pad in (0, 5)]
    _run(3, cases)


@pytest.mark.parametrize("n", [2, 5, 8, 9])
def test_slices_cut_rows(dev, n):
    """1 KiB slices on 4 pipelines, rows of 1028 and 3000 bytes (no slice boundary falls on a row's),
    per-pair counts from {0, 2, 40}: destinations run out at different slices."""
    cases = [dict(C=_pattern(n, (40, 0, 2), i), esz=esz, rowcount=rb // esz, pad=pad, algo=READ, seed=30 + i)
             for i, (rb, esz, pad) in enumerate(((1028, 4, 0), (3000, 2, 0), (3000, 8, 3), (1028, 1, 0)))]
    _run(n, cases, env=SMALL)


@pytest.mark.parametrize("rowcount", [257, 258])
def test_mixed_alignment_in_one_call(dev, rowcount):
    """2-byte elements, rank 1's sendbuff and rank 0's recvbuff 2 bytes off.  258: rank 1 sends elements,
    the others send rank 0 elements and the rest vectors in ONE launch; 257 (no whole dwords): no vectors."""
    cases = [dict(C=_pattern(3, (3, 70, 1), 1), esz=2, rowcount=rowcount, pad=pad, algo=algo, seed=40 + pad,
                  send_off=[0, 2, 0], recv_off=[2, 0, 0]) for pad in (0, 1, 2) for algo in (READ, RING)]
    _run(3, cases)


@pytest.mark.parametrize("n,algo", [(3, READ), (3, RING), (1, READ)])
def test_out_of_range_indices_deliver_zero_rows(dev, n, algo):
    """-1, nrows and INT32_MAX among valid indices, the matrix between marker rows: the rows they name
    arrive as zero bytes -- wide rows, narrow ones, element rows, and the local gather kernel."""
    cases = [dict(C=_pattern(n, (70, 3, 9)), esz=esz, rowcount=rc, pad=2, algo=algo, idx="oob", seed=50 + i,
                  expect_algo=-1 if n == 1 else algo) for i, (esz, rc) in enumerate(((2, 1030), (4, 64), (2, 7), (1, 2051)))]
    _run(n, cases)


@pytest.mark.parametrize("algo", [READ, RING])
def test_identity_indices_agree_with_alltoallv(dev, algo):
    cases = [dict(C=[[5, 0, 9], [9, 5, 1], [3, 9, 5]], esz=esz, rowcount=rc, algo=algo, idx="identity", vs_a2av=True, seed=60)
             for esz, rc in ((2, 1031), (4, 64), (1, 7))]
    _run(3, cases)


def test_graph_replays_read_rowidx_at_replay_time(dev):
    """A captured read-schedule call replayed twice, rowidx rewritten in between: each replay matches the
    indices it ran with.  On a forced ring the capture is ncclInvalidUsage everywhere; the next call is exact."""
    C = _pattern(3, (70, 0, 3, 9))
    cases = [dict(C=C, esz=2, rowcount=1030, pad=1, algo=READ, graph=True, seed=70),
             dict(C=C, esz=4, rowcount=24, algo=READ, graph=True, seed=71),
             dict(C=C, esz=2, rowcount=1030, algo=RING, graph=True, seed=72, want_rc=5),
             dict(C=C, esz=2, rowcount=1030, algo=RING, seed=73)]
    _run(3, cases)


def test_refusals_and_idle_ranks(dev):
    """A rowcount that differs on one rank and a count mismatch: ncclInvalidUsage on every rank, nothing
    written, then a valid call succeeds.  An all-zero matrix launches nothing.  A NULL-buffer rank takes part."""
    n, C = 3, np.array(_pattern(3, (70, 3, 9)))
    idle = C * np.array([1, 0, 1]) * np.array([[1], [0], [1]])  # rank 1 sends and receives nothing
    base = dict(esz=2, rowcount=300, pad=1, algo=READ)  # (the stride leaves room for the rank that passes 301)
    cases = [dict(base, C=C.tolist(), seed=80),
             dict(base, C=C.tolist(), seed=81, bad="rowcount", want_rc=5),
             dict(base, C=C.tolist(), seed=82, bad="count", want_rc=5),
             dict(base, C=C.tolist(), seed=83),
             dict(base, C=np.zeros((n, n), int).tolist(), seed=84, null_ranks=[0, 1, 2]),
             dict(base, C=idle.tolist(), seed=85, null_ranks=[1]),
             dict(base, C=idle.tolist(), seed=86, null_ranks=[1], algo=RING)]
    _run(n, cases)
