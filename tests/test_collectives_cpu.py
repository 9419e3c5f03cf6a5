"""ncclReduceScatter / ncclAllGather without a GPU (-m "not gpu"): the ABI's argument checks, the
ring halves' op tables (csrc/schedule.h coll_op), the simulated kernels' protocol and data on both
schedules -- alone and mixed with all-reduces on one communicator state -- and the new kernels'
resource budget, read from the built library.

Expected values: a reduce-scatter's rank r holds chunk r of the oracle's ring fold (the
all-reduce's bits), an all-gather's every rank holds the concatenation of the inputs.  Inputs are
seeded uniform[-1, 1) fp32 (order-sensitive: another association changes bits).
"""
import ctypes
import re

import numpy as np
import pytest

import oracle_api as O
import sim_api
import sim_coll_api as S
from test_kernel_resources import _disassembly_by_kernel, _kernels

AR, RS, AG = S.ALLREDUCE, S.REDUCE_SCATTER, S.ALLGATHER


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expect(coll, xs, r):
    """What rank r's recv holds after the call over inputs xs (out of place or in place alike)."""
    n = len(xs)
    if coll == AR:
        return O.allreduce(xs, "f32", "sum")[r]
    if coll == RS:
        c = xs[0].size // n
        return O.ring_fold(xs, "f32", "sum")[r * c:(r + 1) * c]
    return np.concatenate(xs)


def _check(coll, xs, outs, what):
    for r in range(len(xs)):
        exp = _expect(coll, xs, r)
        assert np.array_equal(_bits(outs[r]), _bits(exp)), f"{what}: rank {r} differs"


# ---------------------------------------------------------------- the ABI
def test_argument_checks_before_device_work(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced on these paths
    rs = lambda s, r, c, dt, op, comm: L.ncclReduceScatter(s, r, c, dt, op, comm, None)
    ag = lambda s, r, c, dt, comm: L.ncclAllGather(s, r, c, dt, comm, None)
    # NULL comm or buffer, then count == 0 -> success: the all-reduce's order
    assert rs(None, fake, 4, M.ncclFloat, M.ncclSum, fake) == M.ncclInvalidArgument
    assert rs(fake, None, 4, M.ncclFloat, M.ncclSum, fake) == M.ncclInvalidArgument
    assert rs(fake, fake, 4, M.ncclFloat, M.ncclSum, None) == M.ncclInvalidArgument
    assert rs(None, fake, 0, M.ncclFloat, M.ncclSum, fake) == M.ncclInvalidArgument
    assert rs(fake, fake, 0, M.ncclFloat, M.ncclSum, fake) == M.ncclSuccess
    assert rs(fake, fake, 0, M.ncclInt8, M.ncclAvg, fake) == M.ncclSuccess
    assert ag(None, fake, 4, M.ncclFloat, fake) == M.ncclInvalidArgument
    assert ag(fake, None, 4, M.ncclFloat, fake) == M.ncclInvalidArgument
    assert ag(fake, fake, 4, M.ncclFloat, None) == M.ncclInvalidArgument
    assert ag(fake, fake, 0, M.ncclFloat, fake) == M.ncclSuccess
    assert ag(fake, fake, 0, M.ncclInt8, fake) == M.ncclSuccess
    # unsupported dtype or op -> ncclInternalError, before the communicator is touched
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert rs(fake, fake, 4, dt, M.ncclSum, fake) == M.ncclInternalError
        assert ag(fake, fake, 4, dt, fake) == M.ncclInternalError
    assert rs(fake, fake, 4, M.ncclFloat, M.ncclAvg, fake) == M.ncclInternalError
    assert L.mncclVersion() == 600  # the additions are detected by symbol, not by version


def test_symbols_exported_and_bound(nccl_lib):
    import subprocess

    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
    for f in ("ncclReduceScatter", "ncclAllGather"):
        assert f in exported
        assert f in M.SIGNATURES
    assert callable(M.Comm.reduce_scatter) and callable(M.Comm.all_gather)


# ---------------------------------------------------------------- op tables
K_SEND, K_REDUCE_SEND, K_REDUCE_COPY_SEND, K_COPY_SEND, K_COPY = range(5)


@pytest.mark.parametrize("n", range(2, 17))
def test_op_tables(sim_lib, n):
    for coll in (RS, AG):
        nops, mpi = S.num_ops(coll, n), S.msgs_per_iter(coll, n)
        assert (nops, mpi) == ((n + 1, n) if coll == RS else (n, n - 1))
        for r in range(n):
            ops = [S.coll_op(coll, n, r, k) for k in range(nops)]
            sent = [o[2] for o in ops if o[2] >= 0]
            rcvd = [o[3] for o in ops if o[3] >= 0]
            # every rank sends and receives each of the iteration's messages once, in order
            assert sent == list(range(mpi)) and rcvd == list(range(mpi)), (coll, n, r)
            for kind, chunk, _, _ in ops:
                assert 0 <= chunk < n
            kinds = [o[0] for o in ops]
            if coll == RS:
                assert kinds == [K_SEND] + [K_REDUCE_SEND] * (n - 1) + [K_COPY]
                assert ops[0][1] == r and ops[-1][1] == r  # starts its own chunk, ends with it finished
                # every chunk is visited by this rank exactly once as a local operand
                assert sorted(o[1] for o in ops[:-1]) == list(range(n))
            else:
                assert kinds == [K_SEND] + [K_COPY_SEND] * (n - 2) + [K_COPY]
                assert ops[0][1] == r
                assert sorted(o[1] for o in ops) == list(range(n))  # own chunk out, every other one in
            for k, o in enumerate(ops):
                # message m of the sender r - 1 carries the chunk this rank expects in message m
                if o[3] >= 0:
                    prev = [S.coll_op(coll, n, (r - 1) % n, j) for j in range(nops)]
                    src = [p for p in prev if p[2] == o[3]]
                    assert len(src) == 1 and src[0][1] == o[1], (coll, n, r, k)
    # coll 0 is the all-reduce's ring, unchanged
    assert S.num_ops(AR, n) == 2 * n - 1 and S.msgs_per_iter(AR, n) == 2 * (n - 1)
    for r in range(n):
        for k in range(2 * n - 1):
            assert S.coll_op(AR, n, r, k) == S.coll_op(-1, n, r, k)


# ---------------------------------------------------------------- simulator
COUNTS = (1, 255, 256, 1000, 4099)  # floats per chunk: below / at / past a 1 KiB slice, ragged


def _inputs(n, count, seed):
    return O.random_inputs(n, count, "f32", seed=seed)


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9])
def test_sim_halves_alone(sim_lib, oracle_lib, n, channels):
    for c in COUNTS:
        for sched in (S.RING, S.READ):
            for inplace in (False, True):
                xs = _inputs(n, n * c, 100 + c)
                (out,) = S.run(n, [(RS, sched, xs, inplace)], channels=channels, seed=c)
                _check(RS, xs, out, f"reduce-scatter n={n} c={c} sched={sched} inplace={inplace}")
                ys = _inputs(n, c, 200 + c)
                (out,) = S.run(n, [(AG, sched, ys, inplace)], channels=channels, seed=c + 1)
                _check(AG, ys, out, f"all-gather n={n} c={c} sched={sched} inplace={inplace}")


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("sched", [S.RING, S.READ])
def test_sim_reduce_scatter_then_all_gather_is_all_reduce(sim_lib, oracle_lib, n, sched):
    for c in COUNTS:
        xs = _inputs(n, n * c, 300 + c)
        (part,) = S.run(n, [(RS, sched, xs, False)])
        (whole,) = S.run(n, [(AG, sched, part, False)])
        ref, _ = sim_api.allreduce(xs, algo=sched)
        exp = O.allreduce(xs, "f32", "sum")
        for r in range(n):
            assert np.array_equal(_bits(whole[r]), _bits(ref[r])), (n, c, r)
            assert np.array_equal(_bits(whole[r]), _bits(exp[r])), (n, c, r)


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (4, 4), (5, 1), (8, 8), (9, 4)])
def test_sim_mixed_sequence_on_one_state(sim_lib, oracle_lib, n, channels, seed):
    """21 calls on one communicator state: all-reduces on every schedule interleaved with both halves
    on both schedules, sizes changing from call to call.  The ring's FIFOs (slots 2) and the READY /
    CREDIT counters carry over: a half that advanced them by another amount than the kernels'
    peers expect deadlocks or corrupts a later call."""
    oneshot_ok = channels >= n  # a one-shot call needs n pipelines per slice
    plan = [(AR, S.RING), (RS, S.READ), (AG, S.RING), (AR, S.READ), (RS, S.RING), (AG, S.READ),
            (AR, S.ONESHOT if oneshot_ok else S.RING), (AG, S.RING), (RS, S.RING), (AR, S.READ_GRID),
            (RS, S.READ), (RS, S.RING), (AG, S.READ), (AG, S.RING), (AR, S.RING),
            (RS, S.READ), (AR, S.ONESHOT if oneshot_ok else S.READ), (AG, S.READ), (RS, S.RING), (AG, S.RING),
            (AR, S.READ)]
    assert len(plan) == 21
    sizes = (4099, 1, 1000, 256, 255, 700)
    calls, inputs = [], []
    for i, (coll, sched) in enumerate(plan):
        c = 256 if sched == S.ONESHOT else sizes[i % len(sizes)]  # one-shot: one 1 KiB slice per chunk
        count = c if coll == AG else n * c + (3 if coll == AR and sched != S.ONESHOT else 0)
        xs = _inputs(n, count, 1000 * (seed + 1) + i)
        inputs.append(xs)
        calls.append((coll, sched, xs, i % 3 == 1 and not (coll == AR and count % n)))
    outs = S.run(n, calls, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched), xs, out) in enumerate(zip(plan, inputs, outs)):
        _check(coll, xs, out, f"call {i} (coll {coll}, schedule {sched})")


# ---------------------------------------------------------------- kernel resources
def test_new_kernels_fit_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    ks = _kernels(tmp_path)
    fold = {k: v for k, v in ks.items() if "scatter_fold" in k}
    push = {k: v for k, v in ks.items() if "gather_push" in k}
    # scatter_fold: 5 dtypes x 4 ops x (vector, scalar); gather_push: 3 element sizes x (vector, scalar)
    assert len(fold) == 40, sorted(fold)[:5]
    assert len(push) == 6, sorted(push)
    for k, v in {**fold, **push}.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the names stay out of the existing 120-kernel count
    assert not [k for k in {**fold, **push} if re.search(r"(ring|read|oneshot)_kernel", k)]


def test_half_precision_scatter_folds_stay_packed(nccl_lib, tmp_path):
    # the vector path of the F16 / BF16 Sum folds adds pairs: v_pk_add_f16, and v_pk_add_f32 with the
    # packed round back v_cvt_pk_bf16_f32 (as tests/test_kernel_resources.py checks for read_kernel).
    # Counted in the library as built for gfx950 (ROCm 7.2): scatter_fold<_Float16, Sum, vector> holds
    # 488 v_pk_add_f16; scatter_fold<bf16_t, Sum, vector> 464 v_pk_add_f32 and 522 v_cvt_pk_bf16_f32.
    fns = _disassembly_by_kernel(tmp_path)
    for T, ops in (("_Float16", ("v_pk_add_f16",)), ("mnccl::bf16_t", ("v_pk_add_f32", "v_cvt_pk_bf16_f32"))):
        rx = re.compile(r"scatter_fold<" + re.escape(T) + r", 0, true>\(")
        names = [k for k in fns if rx.search(k)]
        assert len(names) == 1, names
        for op in ops:
            c = len(re.findall(r"\s" + op + r"\b", fns[names[0]]))
            assert c >= 1, f"{names[0]}: no {op}"
