"""mncclAllToAllvCombineFp8Block128 on the GPU (-m gpu) against fp8bc_ref.decode under combine_workers.Shape.expect, by bits (NaN as NaN)."""
import pytest

import combine_workers as CW
import combinefp8b_workers as BW
from test_alltoallv_gpu import READ, RING, SMALL, _pattern, dev  # noqa: F401 (dev: the device fixture)
from test_combine_gpu import _run  # the plain combine's runner and verdicts ...

pytestmark = pytest.mark.gpu
ALGOS, DTYPES = [pytest.param(RING, id="ring"), pytest.param(READ, id="read")], ["f32", "f16", "bf16"]


@pytest.fixture(autouse=True)
def fp8b_ranks(monkeypatch):
    monkeypatch.setattr(CW, "combine_rank", BW.combinefp8b_rank)  # ... around this call's rank processes


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_code_sweep(dev, algo, dtype):  # every e4m3 code at each scale word of fp8bc_ref.SCALES: weights NULL, all -0.5
    base = dict(C=[[8, 8], [8, 8]], dtype=dtype, rowcount=256, topk=1, nrows=[200], sweep=True, algo=algo, expect_algo=algo)
    _run(2, [dict(base, weights=False, seed=3), dict(base, w_const=-0.5, seed=4)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ALGOS)
def test_shapes(dev, algo, dtype):  # narrow rows, 24 lanes (no divisor of 64), one pass, partial passes; topk 9: past the group of 8
    _run(3, [dict(C=_pattern(3, (70, 0, 1, 3), i), dtype=dtype, rowcount=rc, pad=pad, topk=(1, 3, 9)[(i + j) % 3],
                  weights=(i + j) % 2 == 0, nrows=[70, 0, 33], algo=algo, expect_algo=algo, seed=10 + 8 * i + pad)
             for i, rc in enumerate((128, 384, 1024, 1152, 2176)) for j, pad in enumerate((0, 6))])


@pytest.mark.parametrize("n", [2, 5, 8])
def test_slices_cut_units(dev, n):  # 1008 = 16 * 63 is no multiple of a unit's 32 (bf16) or 64 (f32) output bytes
    _run(n, [dict(C=_pattern(n, (40, 0, 2), i), dtype=dt, rowcount=rc, pad=pad, topk=k, nrows=[40, 0, 2], algo=READ,
                  expect_algo=READ, seed=50 + i) for i, (rc, dt, pad, k) in enumerate(((384, "bf16", 0, 3), (1152, "f32", 2, 2)))],
         env=dict(SMALL, MINI_NCCL_SLICE_SIZE="1008"))


@pytest.mark.parametrize("algo", ALGOS)
def test_round_trip_with_dispatch(dev, algo):  # the send buffers are what mncclAllToAllvRowsFp8Block128 delivered into them
    _run(3, [dict(C=_pattern(3, (70, 3, 0, 9), i), dtype=dt, rowcount=rc, topk=1, nrows=[70, 9, 33], algo=algo, mx_dispatch=True,
                  expect_algo=algo, seed=70 + i) for i, (dt, rc) in enumerate((("bf16", 1152), ("f32", 128), ("f16", 384)))])


def test_graph_rereads_slots_and_weights(dev):  # on a forced ring the capture is ncclInvalidUsage; the next call is exact
    base = dict(C=_pattern(3, (70, 0, 3, 9)), dtype="bf16", rowcount=1152, pad=2, topk=3, nrows=[70, 0, 33])
    _run(3, [dict(base, algo=READ, expect_algo=READ, graph=True, seed=80),
             dict(base, dtype="f32", rowcount=256, algo=READ, expect_algo=READ, graph=True, seed=81),
             dict(base, algo=RING, graph=True, seed=82, want_rc=5), dict(base, algo=RING, expect_algo=RING, seed=83)])


@pytest.mark.parametrize("n", [3, 1])
def test_refusals_and_the_all_zero_call(dev, n):
    """Local: 4; a datatype without a float: 3; an open group: 5; rank 1 differs: 5 everywhere, then an exact call; no counts at all."""
    base = dict(C=_pattern(n, (70, 3, 9)), dtype="f32", rowcount=384, pad=2, topk=2, nrows=[33, 9, 70], algo=READ, over_all=True)
    local = [dict(rowcount=96, stride=98), dict(rowcount=16512, stride=16512), dict(topk=17), dict(send=None)]
    cases = [dict(base, seed=90 + i, over=o, want_rc=4) for i, o in enumerate(local)]
    cases += [dict(base, seed=100 + i, mx_over=o, want_rc=4) for i, o in enumerate((dict(send_add=2), dict(recv_add=2)))]
    cases += [dict(base, dtype="bf16", seed=102, over=dict(stride=385), want_rc=4),
              dict(base, seed=103, mx_over=dict(dt=2), want_rc=3), dict(base, seed=105, group=True, want_rc=5)]
    base["over_all"] = False
    for i, o in enumerate((dict(mxfp8_on_1=True), dict(mx_over=dict(plain=True)), dict(over=dict(rowcount=256))) if n > 1 else ()):
        cases += [dict(base, seed=114 + i, want_rc=5, **o), dict(base, seed=120 + i)]
    _run(n, cases + [dict(base, seed=112, C=[[0] * n] * n), dict(base, seed=113, dtype="bf16")])
