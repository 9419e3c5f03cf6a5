"""The expectation helpers of tests/lifecycle_workers.py on the CPU: each against a direct numpy
statement of the collective, and the expectations of consecutive replays / rounds against each
other -- they must differ in every chunk, or a stale result could pass."""
import numpy as np
import pytest

import alltoall_workers as AW
import lifecycle_workers as LW
import oracle_api as O

NS = [1, 2, 3, 4, 16]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_elems():
    assert LW.elems("rs", 3, 5) == (15, 5) and LW.elems("ag", 3, 5) == (5, 15) and LW.elems("a2a", 3, 5) == (15, 15)
    assert LW.elems("bc", 3, 5) == LW.elems("rd", 3, 5) == LW.elems("ar", 3, 5) == (5, 5)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype", ["f32", "bf16", "i32"])
def test_copies_against_numpy(oracle_lib, n, dtype):
    """ag: the concatenation; bc: the root's input; a2a: block q of rank r's recv is block r of rank
    q's send (and alltoall_workers.my_expect's bytes); every input has the call's send size."""
    c = 37
    for coll in ("ag", "bc", "a2a"):
        xs = LW.call_inputs(coll, 5, n, c, dtype)
        assert len(xs) == n and all(x.size == LW.elems(coll, n, c)[0] and x.dtype == O.DTYPES[dtype][1] for x in xs)
        for r in range(n):
            e = LW.call_expect(coll, xs, r, dtype, root=n - 1)
            assert e.size == LW.elems(coll, n, c)[1]
            if coll == "ag":
                assert np.array_equal(_bits(e), _bits(np.concatenate(xs)))
            elif coll == "bc":
                assert np.array_equal(_bits(e), _bits(xs[n - 1]))
            else:
                for q in range(n):
                    assert np.array_equal(_bits(e[q * c:(q + 1) * c]), _bits(xs[q][r * c:(r + 1) * c]))
                assert np.array_equal(_bits(e), AW.my_expect(5, r, n, c * e.itemsize))


@pytest.mark.parametrize("n", NS)
def test_reductions_against_numpy(oracle_lib, n):
    """rs: chunk `rank` of the element-wise reduction; rd: all of it on the root, None elsewhere.
    i32 sums (wrapping) and f32 max do not depend on the fold's order, so numpy states them."""
    c = 41
    for dtype, op, fold in (("i32", "sum", lambda xs: np.sum(np.stack(xs).astype(np.int64), axis=0).astype(np.int32)),
                            ("f32", "max", lambda xs: np.maximum.reduce(xs))):
        xs = LW.call_inputs("rs", 9, n, c, dtype)
        whole = fold(xs)
        for r in range(n):
            assert np.array_equal(LW.call_expect("rs", xs, r, dtype, op), whole[r * c:(r + 1) * c])
        ys = LW.call_inputs("rd", 9, n, n * c + 2, dtype)  # a short last chunk
        root = n // 2
        for r in range(n):
            e = LW.call_expect("rd", ys, r, dtype, op, root)
            if r == root:
                assert np.array_equal(e, fold(ys))
            else:
                assert e is None or n == 1


@pytest.mark.parametrize("n", [2, 3, 4])
def test_pairs_against_the_single_calls_and_numpy(oracle_lib, n):
    c = 4099
    root = n - 1
    for pair in ("rs_ag", "rd_bc"):
        xs = LW.pair_inputs(pair, 300, n, c)
        assert all(x.size == n * c for x in xs)
        # the two calls one after the other, from the single-call expectations
        if pair == "rs_ag":
            mids = [LW.call_expect("rs", xs, q, "f32") for q in range(n)]
            via = [LW.call_expect("ag", mids, r, "f32") for r in range(n)]
        else:
            mid = LW.call_expect("rd", xs, root, "f32", "sum", root)
            via = [LW.call_expect("bc", [mid] * n, r, "f32", root=root) for r in range(n)]
        for r in range(n):
            assert np.array_equal(_bits(LW.pair_expect(pair, xs, r)), _bits(via[r]))
        # integer-valued floats: every order of the sum is exact, numpy states it
        ints = [np.rint(x * 1000).astype(np.float32) for x in xs]
        for r in range(n):
            assert np.array_equal(LW.pair_expect(pair, ints, r), np.sum(np.stack(ints), axis=0, dtype=np.float64).astype(np.float32))
    xs = LW.pair_inputs("a2a_a2a", 300, n, c)
    once = [LW.call_expect("a2a", xs, r, "f32") for r in range(n)]
    for r in range(n):
        assert np.array_equal(_bits(LW.call_expect("a2a", once, r, "f32")), _bits(xs[r]))
        assert np.array_equal(_bits(LW.pair_expect("a2a_a2a", xs, r)), _bits(xs[r]))


def _every_chunk_differs(a, b, chunk):
    assert a.size == b.size
    for lo in range(0, a.size, chunk):
        if np.array_equal(_bits(a[lo:lo + chunk]), _bits(b[lo:lo + chunk])):
            return False
    return True


@pytest.mark.parametrize("coll", LW.FIVE + ("ar",))
def test_consecutive_replays_expect_other_data_in_every_chunk(oracle_lib, coll):
    """graph_rank's seeds (seed, seed + 1000, ...) and cases_rank's / threaded_colls_proc's (+ 1 per
    call): the expectation of every rank, and its own send, change in every chunk of `count`
    elements from one replay to the next -- a result left over from the previous one cannot pass."""
    n, root = 3, 1
    c = 3 * 257 + 2 if coll in ("bc", "rd", "ar") else 257
    chunk = (c + n - 1) // n if coll in ("bc", "rd", "ar") else c
    for step in (1000, 1):
        prev = None
        for k in range(5):
            xs = LW.call_inputs(coll, 100 + step * k, n, c, "f32")
            cur = (xs, [LW.call_expect(coll, xs, r, "f32", "sum", root) for r in range(n)])
            if prev is not None:
                for r in range(n):
                    assert _every_chunk_differs(prev[0][r], cur[0][r], chunk), (coll, k, r)
                    if cur[1][r] is not None:
                        assert _every_chunk_differs(prev[1][r], cur[1][r], chunk), (coll, k, r)
            prev = cur


@pytest.mark.parametrize("pair", LW.PAIRS)
def test_consecutive_rounds_of_a_pair_expect_other_data_in_every_chunk(oracle_lib, pair):
    """graph_pair_rank's seeds (300, 301, ...) and chains_rank's (700 + 10 * round + chain)."""
    n, c = 3, 257
    for seeds in ((300, 301, 302, 303), (700, 710), (701, 711), (702, 712)):
        prev = None
        for s in seeds:
            xs = LW.pair_inputs(pair, s, n, c)
            cur = [LW.pair_expect(pair, xs, r) for r in range(n)]
            if prev is not None:
                for r in range(n):
                    assert _every_chunk_differs(prev[r], cur[r], c), (pair, s, r)
            prev = cur
