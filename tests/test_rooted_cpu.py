"""ncclBroadcast / ncclReduce without a GPU (-m "not gpu"): the ABI's argument checks, the ring's
rooted op tables (csrc/schedule.h coll_op with a root), the simulated kernels' protocol and data
on both schedules -- alone, composed, and mixed with the three other collectives on one
communicator state -- and the new kernels' resource budget, read from the built library.

Expected values (rooted_ref.py): a Reduce's root holds, per chunk c of ceil(count / n) elements,
the oracle's fold acc = x_c, acc = op(x_k, acc) for k = c + 1, ..., c - 1; a Broadcast's every rank
holds the root's input.  Inputs are seeded uniform[-1, 1) fp32 (order-sensitive: another
association changes bits).  Everything is compared bit for bit.
"""
import ctypes
import re

import numpy as np
import pytest

import oracle_api as O
import rooted_ref
import sim_api
import sim_rooted_api as R
from test_kernel_resources import _kernels

AR, RS, AG, BC, RD = R.ALLREDUCE, R.REDUCE_SCATTER, R.ALLGATHER, R.BROADCAST, R.REDUCE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(n, count, seed):
    return O.random_inputs(n, count, "f32", seed=seed)


def _check(coll, xs, root, outs, spares, what):
    """One call's result on the ranks the collective defines, and its sentinel buffers."""
    n = len(xs)
    if coll == AR:
        exp = O.allreduce(xs, "f32", "sum")
        for r in range(n):
            assert np.array_equal(_bits(outs[r]), _bits(exp[r])), f"{what}: rank {r} differs"
    elif coll == RS:
        c = xs[0].size // n
        exp = O.ring_fold(xs, "f32", "sum")
        for r in range(n):
            assert np.array_equal(_bits(outs[r]), _bits(exp[r * c:(r + 1) * c])), f"{what}: rank {r} differs"
    elif coll == AG:
        for r in range(n):
            assert np.array_equal(_bits(outs[r]), _bits(np.concatenate(xs))), f"{what}: rank {r} differs"
    elif coll == BC:
        for r in range(n):
            assert np.array_equal(_bits(outs[r]), _bits(xs[root])), f"{what}: rank {r} differs"
    else:
        assert np.array_equal(_bits(outs[root]), _bits(rooted_ref.reduce_expect(xs))), f"{what}: the root differs"
    for r, spare in enumerate(spares):
        if spare is not None:
            assert np.all(spare == R.SENTINEL), f"{what}: rank {r}'s unused buffer was written"


# ---------------------------------------------------------------- the ABI
def test_argument_checks_before_device_work(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced on these paths
    bc = lambda s, r, c, dt, root, comm: L.ncclBroadcast(s, r, c, dt, root, comm, None)
    rd = lambda s, r, c, dt, op, root, comm: L.ncclReduce(s, r, c, dt, op, root, comm, None)
    # NULL comm, then count == 0 -> success before the datatype or the communicator is looked at
    assert bc(fake, fake, 4, M.ncclFloat, 0, None) == M.ncclInvalidArgument
    assert rd(fake, fake, 4, M.ncclFloat, M.ncclSum, 0, None) == M.ncclInvalidArgument
    assert bc(fake, fake, 0, M.ncclFloat, 0, None) == M.ncclInvalidArgument
    assert bc(fake, fake, 0, M.ncclInt8, 0, fake) == M.ncclSuccess
    assert bc(None, None, 0, M.ncclInt8, 99, fake) == M.ncclSuccess
    assert rd(fake, fake, 0, M.ncclInt8, M.ncclAvg, 0, fake) == M.ncclSuccess
    assert rd(None, None, 0, M.ncclFloat, M.ncclSum, -1, fake) == M.ncclSuccess
    # unsupported dtype or op -> ncclInternalError, before the communicator is touched
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert bc(fake, fake, 4, dt, 0, fake) == M.ncclInternalError
        assert rd(fake, fake, 4, dt, M.ncclSum, 0, fake) == M.ncclInternalError
    assert rd(fake, fake, 4, M.ncclFloat, M.ncclAvg, 0, fake) == M.ncclInternalError
    assert L.mncclVersion() == 600  # the additions are detected by symbol, not by version


def test_symbols_exported_and_bound(nccl_lib):
    import subprocess

    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    for f in ("ncclBroadcast", "ncclReduce"):
        assert f in exported
        assert f in M.SIGNATURES
    assert len(M.SIGNATURES["ncclBroadcast"][1]) == 7 and len(M.SIGNATURES["ncclReduce"][1]) == 8
    assert callable(M.Comm.broadcast) and callable(M.Comm.reduce)


# ---------------------------------------------------------------- op tables
K_SEND, K_REDUCE_SEND, K_REDUCE_COPY_SEND, K_COPY_SEND, K_COPY, K_FORWARD, K_DROP = range(7)
STORES_RECV = (K_REDUCE_COPY_SEND, K_COPY_SEND, K_COPY)


@pytest.mark.parametrize("n", range(2, 17))
def test_rooted_op_tables(sim_lib, n):
    S = R.S
    for root in range(n):
        # ---- Broadcast: a chain root -> root+1 -> ... -> root-1, one op per iteration
        assert S.num_ops(BC, n) == 1 and S.msgs_per_iter(BC, n) == 1
        for r in range(n):
            kind, chunk, send_msg, recv_msg = R.coll_op(BC, n, r, 0, root)
            pos = (r - root) % n
            assert chunk == 0  # the whole buffer is one chunk
            assert kind == (K_SEND if pos == 0 else K_COPY if pos == n - 1 else K_COPY_SEND), (n, root, r)
            assert (send_msg, recv_msg) == (0 if pos < n - 1 else -1, 0 if pos > 0 else -1)
            # each link's sends equal its peer's receives, per iteration (root-1 -> root: nothing)
            assert R.tx_msgs(BC, n, r, root) == (1 if send_msg >= 0 else 0)
            assert R.rx_msgs(BC, n, r, root) == (1 if recv_msg >= 0 else 0)
            assert R.tx_msgs(BC, n, r, root) == R.rx_msgs(BC, n, (r + 1) % n, root), (n, root, r)
        # ---- Reduce: the all-reduce's table; no kind that stores to recv off the root
        nops = S.num_ops(RD, n)
        assert nops == 2 * n - 1 and S.msgs_per_iter(RD, n) == 2 * (n - 1)
        for r in range(n):
            ops = [R.coll_op(RD, n, r, k, root) for k in range(nops)]
            ref = [S.coll_op(AR, n, r, k) for k in range(nops)]
            assert [o[1:] for o in ops] == [o[1:] for o in ref]  # chunks and messages: the all-reduce's
            assert R.tx_msgs(RD, n, r, root) == R.rx_msgs(RD, n, (r + 1) % n, root) == 2 * (n - 1)
            assert sorted(o[2] for o in ops if o[2] >= 0) == list(range(2 * (n - 1)))
            assert sorted(o[3] for o in ops if o[3] >= 0) == list(range(2 * (n - 1)))
            if r == root:
                assert ops == ref
                # the root stores every chunk of its recv exactly once
                assert sorted(o[1] for o in ops if o[0] in STORES_RECV) == list(range(n))
            else:
                mask = {K_REDUCE_COPY_SEND: K_REDUCE_SEND, K_COPY_SEND: K_FORWARD, K_COPY: K_DROP}
                assert [o[0] for o in ops] == [mask.get(o[0], o[0]) for o in ref]
                assert not [o for o in ops if o[0] in STORES_RECV], (n, root, r)
    # the unrooted tables do not depend on the root argument
    for coll in (AR, RS, AG):
        for r in range(n):
            for k in range(S.num_ops(coll, n)):
                assert R.coll_op(coll, n, r, k, n - 1) == S.coll_op(coll, n, r, k)
            assert R.tx_msgs(coll, n, r, 1) == R.rx_msgs(coll, n, r, 1) == S.msgs_per_iter(coll, n)


def test_rooted_len_clamps_to_the_buffer(sim_lib):
    # 10 elements on 4 ranks: q = 3, chunks of 3, 3, 3, 1 elements; 8-byte slices
    total, cb = 40, 12
    got = [[R.rooted_len(total, c * cb, cb, 8, s) for s in range(3)] for c in range(4)]
    assert got == [[8, 4, 0], [8, 4, 0], [8, 4, 0], [4, 0, 0]]
    # 3 elements on 4 ranks: the last chunk is empty
    assert [R.rooted_len(12, c * 4, 4, 1024, 0) for c in range(4)] == [4, 4, 4, 0]
    assert R.rooted_len(12, 16, 4, 1024, 0) == 0  # past the end


# ---------------------------------------------------------------- simulator
def _counts(n):
    return (1, n - 1, n, n + 1, 300, 4099, 16411)  # n - 1: an empty chunk


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16])
def test_sim_rooted_alone(sim_lib, oracle_lib, n):
    """Both schedules, roots 0 / 1 / n-1, in place and out of place on the root, 1 KiB slices on 4
    pipelines.  Non-roots pass NULL (odd ranks) or a sentinel buffer (even ranks) for the side their
    role does not use; a sentinel-filled non-root Reduce recv must come back unchanged."""
    for c in _counts(n):
        xs = _inputs(n, c, 100 + c)
        for root in sorted({0, 1, n - 1}):
            for sched in (R.RING, R.READ):
                for inplace in (False, True):
                    for coll in (BC, RD):
                        what = f"coll {coll} n={n} count={c} root={root} sched={sched} inplace={inplace}"
                        (out,) = R.run(n, [(coll, sched, xs, inplace, root)], seed=c + root)
                        _check(coll, xs, root, out, R.last_spares[0], what)
                        if coll == RD:  # the sentinel recvs are the returned buffers themselves
                            for r in range(n):
                                if r != root and out[r] is not None:
                                    assert np.all(out[r] == R.SENTINEL), f"{what}: rank {r}'s recv was written"


@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("sched", [R.RING, R.READ])
def test_sim_reduce_is_the_all_reduce_on_the_root(sim_lib, oracle_lib, n, sched):
    for c in (1, 255, 256, 1000, 4099):
        xs = _inputs(n, n * c, 300 + c)
        ref, _ = sim_api.allreduce(xs, algo=sched)
        exp = O.allreduce(xs, "f32", "sum")
        for root in (0, n - 1):
            (red,) = R.run(n, [(RD, sched, xs, False, root)])
            assert np.array_equal(_bits(red[root]), _bits(ref[root])), (n, c, root)
            assert np.array_equal(_bits(red[root]), _bits(exp[root])), (n, c, root)
            # Reduce(root) then Broadcast(root) = the all-reduce on every rank
            ys = [red[root] if r == root else np.zeros(n * c, np.float32) for r in range(n)]
            (whole,) = R.run(n, [(BC, sched, ys, False, root)])
            for r in range(n):
                assert np.array_equal(_bits(whole[r]), _bits(exp[r])), (n, c, root, r)


@pytest.mark.parametrize("seed", [0, 1, 7, 12])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (4, 4), (5, 1), (8, 8), (9, 4)])
def test_sim_mixed_sequence_on_one_state(sim_lib, oracle_lib, n, channels, seed):
    """12 random calls on one communicator state mixing all five collectives, both schedules and
    changing roots.  The ring's FIFOs (slots 2) and the READY / CREDIT counters carry over: a
    Broadcast whose links advanced by another amount than their peers expect -- its root-1 -> root
    link carries nothing -- deadlocks or corrupts a later call."""
    g = np.random.default_rng(1000 * n + seed)
    sizes = (4099, 1, 1000, 256, 255, 700, n - 1, n + 1)
    calls, meta = [], []
    for i in range(12):
        coll = int(g.integers(0, 5)) if i >= 5 else (BC, RD, AR, RS, AG)[(i + seed) % 5]
        sched = int(g.choice([R.RING, R.READ]))
        root = int(g.integers(0, n))
        c = int(sizes[int(g.integers(0, len(sizes)))])
        count = c if coll in (AG, BC, RD) else n * c + (3 if coll == AR else 0)
        inplace = bool(g.integers(0, 2)) and not (coll == AR and count % n)
        xs = _inputs(n, count, 5000 * (seed + 1) + i)
        calls.append((coll, sched, xs, inplace, root))
        meta.append((coll, sched, xs, root))
    outs = R.run(n, calls, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched, xs, root), out) in enumerate(zip(meta, outs)):
        _check(coll, xs, root, out, R.last_spares[i], f"call {i} (coll {coll}, schedule {sched}, root {root})")


# ---------------------------------------------------------------- kernel resources
def test_rooted_kernels_fit_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    ks = _kernels(tmp_path)
    fold = {k: v for k, v in ks.items() if "root_fold" in k}
    relay = {k: v for k, v in ks.items() if "root_relay" in k}
    # root_fold: 5 dtypes x 4 ops x (vector, scalar); root_relay: 3 element sizes x (vector, scalar)
    assert len(fold) == 40, sorted(fold)[:5]
    assert len(relay) == 6, sorted(relay)
    for k, v in {**fold, **relay}.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the names stay out of the existing 120-kernel count
    assert not [k for k in {**fold, **relay} if re.search(r"(ring|read|oneshot)_kernel", k)]
