"""mncclAllToAllvRowsMxfp8 on the GPU (-m gpu) against mx_ref.quantise of numpy's gather, byte for byte, guards included."""
import numpy as np
import pytest

import gpu_workers as GW
import rowsmx_workers as MW
from test_alltoallv_gpu import ENV, READ, RING, SMALL, _pattern, dev  # noqa: F401 (dev: the device fixture)

pytestmark = pytest.mark.gpu


def _run(n, cases, env=None):
    port, e = GW.free_port(), dict(ENV, **(env or {}))
    out = GW.run_ranks(MW.mx_rank, n, lambda r: (r, n, port, cases, e), 240, barrier=True)
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
            if want == 0:
                assert res["algos"] == [c.get("expect_algo", c["algo"])] * (2 if c.get("graph") else 1), (r, c, res["algos"])


@pytest.mark.parametrize("n", [pytest.param(1, id="pack"), pytest.param(2, id="push")])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_exhaustive_encode(dev, n, dtype):
    """mx_ref.sweep as 28 rows of 16384 elements: saturation, underflow, subnormal inputs, NaN / inf blocks."""
    C = [[28]] if n == 1 else [[14, 14], [14, 14]]
    _run(n, [dict(C=C, rowcount=16384, idx="identity", sweep=True, dtype=dtype, algo=READ, seed=1,
                  expect_algo=-1 if n == 1 else READ)])


@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_shapes(dev, algo):
    """Top-2 indices: narrow rows, one pass, a pass and a partial one, a 224-byte strip, the strip's maximum."""
    cases = [dict(C=_pattern(3, (70, 0, 1, 3), i), rowcount=rc, pad=pad, algo=algo, seed=10 * i + pad, dtype=("bf16", "f16")[i % 2])
             for i, rc in enumerate((128, 1024, 1152, 7168, 16384)) for pad in (0, 6)]
    _run(3, cases)


@pytest.mark.parametrize("n", [2, 8])
def test_slices_cut_records(dev, n):
    """1 KiB slices on 4 pipelines, records of 132 and 1188 bytes, per-pair counts from {0, 2, 40}."""
    cases = [dict(C=_pattern(n, (40, 0, 2), i), rowcount=rc, algo=READ, seed=30 + i) for i, rc in enumerate((128, 1152))]
    _run(n, cases, env=SMALL)


@pytest.mark.parametrize("n,algo", [(3, READ), (1, READ)])
def test_out_of_range_indices_deliver_zero_records(dev, n, algo):
    cases = [dict(C=_pattern(n, (70, 3, 9)), rowcount=rc, pad=2, algo=algo, idx="oob", seed=50 + i,
                  expect_algo=-1 if n == 1 else algo) for i, rc in enumerate((2048, 256))]
    _run(n, cases)


def test_graph_replays_read_rowidx_at_replay_time(dev):
    C = _pattern(3, (70, 0, 3, 9))
    _run(3, [dict(C=C, rowcount=1152, pad=2, algo=READ, graph=True, seed=70),
             dict(C=C, rowcount=1152, algo=RING, graph=True, seed=72, want_rc=5),
             dict(C=C, rowcount=1152, algo=RING, seed=73)])


def test_refusals_and_idle_ranks(dev):
    """Local refusals (4; f32: 3), the rendezvous' (5 everywhere, then an exact call), all-zero counts, a NULL-buffer rank."""
    n, C = 3, np.array(_pattern(3, (70, 3, 9)))
    idle = C * np.array([1, 0, 1]) * np.array([[1], [0], [1]])  # rank 1 sends and receives nothing
    base = dict(rowcount=256, pad=128, algo=READ, C=C.tolist())
    cases = [dict(base, rowcount=96, want_rc=4), dict(base, rowcount=16512, want_rc=4), dict(base, recv_off=2, want_rc=4),
             dict(base, dtype="f32", want_rc=3), dict(base, seed=80),
             dict(base, seed=81, bad="rowcount", want_rc=5), dict(base, seed=82, bad="count", want_rc=5), dict(base, seed=83),
             dict(base, C=np.zeros((n, n), int).tolist(), seed=84, null_ranks=[0, 1, 2]),
             dict(base, C=idle.tolist(), seed=85, null_ranks=[1]), dict(base, C=idle.tolist(), seed=86, null_ranks=[1], algo=RING)]
    _run(n, cases)
