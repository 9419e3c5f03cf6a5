"""mncclAllToAllvRowsFp8Block128 on the GPU (-m gpu) against fp8b_ref.quantise of numpy's gather, byte for byte, guards included."""
import numpy as np
import pytest

import rowsfp8b_workers as W
import rowsmx_workers as MW
from test_alltoallv_gpu import READ, RING, SMALL, _pattern, dev  # noqa: F401 (dev: the device fixture)
from test_rowsmx_gpu import _run  # the MXFP8 suite's runner and verdicts ...

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fp8b_ranks(monkeypatch):
    monkeypatch.setattr(MW, "mx_rank", W.fp8b_rank)  # ... around this call's rank processes


@pytest.mark.parametrize("n", [pytest.param(1, id="pack"), pytest.param(2, id="push")])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_exhaustive_encode(dev, n, dtype):  # fp8b_ref.sweep as 28 rows of 16384 elements
    _run(n, [dict(C=[[28]] if n == 1 else [[14, 14], [14, 14]], rowcount=16384, idx="identity", sweep=True, dtype=dtype, algo=READ, seed=1,
                  expect_algo=-1 if n == 1 else READ)])


@pytest.mark.parametrize("algo", [pytest.param(RING, id="ring"), pytest.param(READ, id="read")])
def test_shapes(dev, algo):  # 8 lanes per row, 8 rows a pass, one scale; 16 lanes; one pass of 8 groups; a pass and a partial one of a single group; 2 passes and a group; a 224-byte strip; the whole strip.  200 records: over 3 index batches of 64
    cases = [dict(C=_pattern(3, (200, 0, 1, 67), i), rowcount=rc, pad=pad, algo=algo, seed=10 * i + pad, dtype=("bf16", "f16")[i % 2])
             for i, rc in enumerate((128, 256, 1024, 1152, 2176, 7168, 16384)) for pad in (0, 6)]
    _run(3, cases)


@pytest.mark.parametrize("n", [2, 8])
def test_slices_cut_records(dev, n):
    cases = [dict(C=_pattern(n, (40, 0, 2), i), rowcount=rc, algo=READ, seed=30 + i) for i, rc in enumerate((128, 1152))]
    _run(n, cases, env=SMALL)


@pytest.mark.parametrize("n,algo", [(3, READ), (1, READ)])
def test_out_of_range_indices_deliver_zero_records(dev, n, algo):  # scale 1e-4f / 448.0f, zero bytes
    cases = [dict(C=_pattern(n, (70, 3, 9)), rowcount=rc, pad=2, algo=algo, idx="oob", seed=50 + i,
                  expect_algo=-1 if n == 1 else algo) for i, rc in enumerate((2048, 256))]
    _run(n, cases)


def test_graph_replays_read_rowidx_at_replay_time(dev):
    C = _pattern(3, (70, 0, 3, 9))
    _run(3, [dict(C=C, rowcount=1152, pad=2, algo=READ, graph=True, seed=70),
             dict(C=C, rowcount=1152, algo=RING, graph=True, seed=72, want_rc=5), dict(C=C, rowcount=1152, algo=RING, seed=73)])


def test_refusals_and_idle_ranks(dev):
    n, C = 3, np.array(_pattern(3, (70, 3, 9)))
    idle = C * np.array([1, 0, 1]) * np.array([[1], [0], [1]])  # rank 1 sends and receives nothing
    base = dict(rowcount=256, pad=128, algo=READ, C=C.tolist())
    cases = [dict(base, rowcount=96, want_rc=4), dict(base, rowcount=16512, want_rc=4), dict(base, recv_off=2, want_rc=4),
             dict(base, dtype="f32", want_rc=3), dict(base, seed=80),
             dict(base, seed=81, bad="rowcount", want_rc=5), dict(base, seed=82), dict(base, seed=83, bad="mxfp8", want_rc=5),
             dict(base, seed=84), dict(base, C=np.zeros((n, n), int).tolist(), seed=85, null_ranks=[0, 1, 2]),
             dict(base, C=idle.tolist(), seed=86, null_ranks=[1]), dict(base, C=idle.tolist(), seed=87, null_ranks=[1], algo=RING)]
    _run(n, cases)
