"""ncclGather / ncclScatter without a GPU (-m "not gpu"): the ABI's checks that need no
communicator, the ring's two chain tables (csrc/schedule.h coll_op, coll_tx_msgs / coll_rx_msgs,
coll_num_ops), the simulated kernels' protocol and data on both schedules -- alone and mixed with the
seven other collectives on one communicator state -- and the two new kernels' resource budget, read
from the library.

The expected result is the permutation itself (sim_gather_scatter_api.gather_expect /
scatter_expect): the root's recv is the ranks' blocks in rank order; rank q's recv is block q of the
root's send.  Buffers are seeded random BYTES compared as bytes; sim_gather_scatter_api.run checks
after every call the guards around every buffer, the sends, and the buffers the non-roots passed
for the side their role does not use (NULL on odd ranks).

The ring and one slot: both chains have kForward ops from 3 ranks on, and with one slot a kForward's
send waits for a credit -- but a chain has an end that only consumes, so unlike the all-reduce's ring
it cannot close a cycle: one slot runs at every rank count, on both schedules.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import sim_gather_scatter_api as G
from test_kernel_resources import _kernels

AR, RS, AG, BC, RD, A2A, A2AV, GA, SC = range(9)
K_SEND, K_COPY, K_FORWARD = 0, 4, 5


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_bound(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    for f in ("ncclGather", "ncclScatter"):
        assert f in exported
        assert f in M.SIGNATURES and len(M.SIGNATURES[f][1]) == 7
    assert callable(M.Comm.gather) and callable(M.Comm.scatter)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version


@pytest.mark.parametrize("name", ["ncclGather", "ncclScatter"])
def test_argument_checks_before_device_work(nccl_lib, name):
    import mini_nccl as M
    fn = getattr(nccl_lib, name)
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)  # never dereferenced on these paths
    call = lambda s, r, c, dt, root, comm: fn(s, r, c, dt, root, comm, None)
    # 1. a NULL comm, before anything else (a count of 0 and a bad datatype included)
    assert call(fake, other, 4, M.ncclFloat, 0, None) == M.ncclInvalidArgument
    assert call(fake, other, 0, M.ncclInt8, 0, None) == M.ncclInvalidArgument
    # 2. count == 0 -> success before the datatype, the root or the communicator is looked at; the
    #    buffers are not looked at either (either may be NULL off the root)
    assert call(fake, other, 0, M.ncclFloat, 0, fake) == M.ncclSuccess
    assert call(fake, other, 0, M.ncclInt8, 0, fake) == M.ncclSuccess
    assert call(fake, other, 0, M.ncclFloat, -1, fake) == M.ncclSuccess
    assert call(fake, other, 0, M.ncclInt8, 99, fake) == M.ncclSuccess
    assert call(None, None, 0, M.ncclFloat, 0, fake) == M.ncclSuccess
    # 4. unsupported datatype -> ncclInternalError, before the communicator is touched (and before
    #    the root and the buffers, which need it)
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert call(fake, other, 4, dt, 0, fake) == M.ncclInternalError
        assert call(None, None, 4, dt, -1, fake) == M.ncclInternalError


@pytest.mark.parametrize("name", ["ncclGather", "ncclScatter"])
def test_inside_an_open_group(nccl_lib, name):
    import mini_nccl as M
    L = nccl_lib
    fn = getattr(L, name)
    fake = ctypes.c_void_p(0x1000)
    assert L.ncclGroupStart() == 0
    try:
        # 3. a group is open: ncclInvalidUsage with nothing launched (the fake communicator is never
        #    read) -- after the NULL comm and the count of 0, before the datatype
        assert fn(fake, fake, 4, M.ncclFloat, 0, fake, None) == M.ncclInvalidUsage
        assert fn(fake, fake, 4, M.ncclInt8, 0, fake, None) == M.ncclInvalidUsage
        assert fn(fake, fake, 4, M.ncclFloat, 0, None, None) == M.ncclInvalidArgument
        assert fn(fake, fake, 0, M.ncclInt8, 0, fake, None) == M.ncclSuccess
        # the group stays open, clean and usable: a count-0 send records nothing, the end succeeds
        assert L.ncclSend(fake, 0, M.ncclFloat, 1, fake, None) == M.ncclSuccess
    finally:
        rc = L.ncclGroupEnd()
    assert rc == M.ncclSuccess
    assert L.ncclGroupEnd() == M.ncclInvalidUsage  # and is closed now
    assert fn(fake, fake, 4, M.ncclInt8, 0, fake, None) == M.ncclInternalError  # as with no group before


# ---------------------------------------------------------------- ring tables
NS_TABLE = list(range(2, 17))


def _tables(coll, n, root):
    return [[G.V.A.R.coll_op(coll, n, r, k, root) for k in range(G.num_ops_at(coll, n, r, root))] for r in range(n)]


@pytest.mark.parametrize("coll", [GA, SC], ids=["gather", "scatter"])
@pytest.mark.parametrize("n", NS_TABLE)
def test_ring_tables(sim_lib, coll, n):
    R = G.V.A.R
    G.load()
    assert R.S.num_ops(coll, n) == n - 1  # the exported rootless form answers with the root's count
    for root in range(n):
        tables = _tables(coll, n, root)
        silent = root if coll == GA else (root - 1) % n  # the link r -> r+1 that carries nothing
        for r in range(n):
            tx, rx_next = R.tx_msgs(coll, n, r, root), R.rx_msgs(coll, n, (r + 1) % n, root)
            assert tx == rx_next, (n, root, r)  # sender and receiver of every link agree
            assert (tx == 0) == (r == silent), (n, root, r)
            pos = (r - root) % n
            assert tx == (pos if coll == GA else n - 1 - pos)
            # send_msg and recv_msg each run 0, 1, 2, ... in op order, and count what the links carry
            assert [o[2] for o in tables[r] if o[2] >= 0] == list(range(tx))
            assert [o[3] for o in tables[r] if o[3] >= 0] == list(range(R.rx_msgs(coll, n, r, root)))
            assert len(tables[r]) == (n - 1 if pos == 0 else pos if coll == GA else n - pos)
        # follow every kSend hop by hop to the kCopy that ends it
        by_recv = [{o[3]: o for o in t if o[3] >= 0} for t in tables]
        delivered = {}
        for s in range(n):
            for kind, block, msg, _ in tables[s]:
                if kind != K_SEND:
                    continue
                at, hops = (s + 1) % n, 1
                while True:
                    o = by_recv[at][msg]
                    if o[0] == K_COPY:
                        break
                    assert o[0] == K_FORWARD and hops < n
                    at, msg, hops = (at + 1) % n, o[2], hops + 1
                assert (block, at) not in delivered
                delivered[(block, at)] = o[1]
        if coll == GA:
            # every block but the root's reaches the root exactly once, into the block of its rank
            assert delivered == {(q, root): q for q in range(n) if q != root}
        else:
            # every block but the root's reaches its owner exactly once (chunk: the shifted recv's block)
            assert delivered == {(q, q): q for q in range(n) if q != root}
        kinds = {o[0] for t in tables for o in t}
        assert kinds <= {K_SEND, K_COPY, K_FORWARD}


# ---------------------------------------------------------------- simulator
def _roots(n):
    return list(range(n)) if n == 3 else [0, n - 1]


def _one(coll, n, root, sched, count, inplace, channels, slots, seed, calls=2):
    """`calls` calls in a row on one state (fresh bytes each): a call whose counters ended out of step
    with its peers' deadlocks or corrupts the next."""
    if coll == GA:
        ins = [G.gather_inputs(n, 4 * count, 1000 * seed + i) for i in range(calls)]
    else:
        ins = [G.scatter_input(n, 4 * count, 1000 * seed + i) for i in range(calls)]
    outs = G.run(n, [(coll, sched, x, inplace, root) for x in ins], slice_bytes=1024, channels=channels, slots=slots,
                 seed=seed)
    what = f"coll={coll} n={n} root={root} sched={sched} count={count} inplace={inplace} K={slots} seed={seed}"
    for i, (x, out) in enumerate(zip(ins, outs)):
        if coll == GA:
            assert np.array_equal(out, G.gather_expect(x)), f"{what} call {i}: the root's recv differs"
        else:
            for q, e in enumerate(G.scatter_expect(x, n)):
                assert np.array_equal(out[q], e), f"{what} call {i}: rank {q} differs"


@pytest.mark.parametrize("sched", [G.RING, G.READ], ids=["ring", "read"])
@pytest.mark.parametrize("coll", [GA, SC], ids=["gather", "scatter"])
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_sim_gather_scatter(sim_lib, n, coll, sched):
    """1 KiB slices on 4 pipelines; counts 1, 300 and 16411 per block; out of place and in place on
    the root; slots 1 and 2; several schedule seeds (0 is the round-robin order).  Exact, no deadlock,
    the non-roots' unused buffers untouched, and a second call on the same state exact too."""
    for root in _roots(n):
        for count in (1, 300, 16411):
            for inplace in (False, True):
                for seed in (0, 1, 2, 5, 11):
                    _one(coll, n, root, sched, count, inplace, 4, (1, 2)[seed % 2], seed)


def test_sim_one_rank(sim_lib):
    for coll in (GA, SC):
        for sched in (G.RING, G.READ):
            for inplace in (False, True):
                _one(coll, 1, 0, sched, 300, inplace, 4, 2, 0, calls=1)


def _check(coll, xs, root, out, what):
    from test_rooted_cpu import _check as check_other
    n = len(out) if coll != GA else None
    if coll == GA:
        assert np.array_equal(out, G.gather_expect(xs)), f"{what}: the root's recv differs"
    elif coll == SC:
        for q, e in enumerate(G.scatter_expect(xs, n)):
            assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
    elif coll == A2A:
        for q, e in enumerate(G.V.A.expect(xs)):
            assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
    elif coll == A2AV:
        lay, sends = xs
        for q, e in enumerate(lay.expect(sends)):
            assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
    else:
        check_other(coll, xs, root, out, [None] * len(xs), what)


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (5, 1), (8, 8), (9, 4)])
def test_sim_all_nine_on_one_state(sim_lib, oracle_lib, n, channels, seed):
    """20 calls on one communicator state mixing all nine collectives and both schedules, the root
    changing every call: the first nine are one of each, every other later call a gather or a scatter,
    the rest random.  No deadlock and every call exact -- the chains' uneven per-link counts stay in
    step with every other collective's."""
    import oracle_api as O
    g = np.random.default_rng(9000 * n + seed)
    sizes = (4099, 1, 1000, 256, 255, 700, 3)
    calls = []
    for i in range(20):
        coll = (i + seed) % 9 if i < 9 else (GA, SC)[(i // 2) % 2] if i % 2 else int(g.integers(0, 9))
        # (the later gathers and scatters: each on the ring and on the read schedule, whatever the seed)
        sched = (G.RING, G.READ)[(i // 4) % 2 if i >= 9 and i % 2 else (i + seed) % 2]
        root = (i + seed) % n
        c = int(sizes[int(g.integers(0, len(sizes)))])
        inplace = bool(g.integers(0, 2)) if coll in (GA, SC) else False
        if coll == GA:
            xs = G.gather_inputs(n, 4 * c, 100 * seed + i)
        elif coll == SC:
            xs = G.scatter_input(n, 4 * c, 100 * seed + i)
        elif coll == A2A:
            xs = G.V.A.random_blocks(n, 4 * c, 100 * seed + i)
        elif coll == A2AV:
            lay = G.V.Layout(G.V.random_matrix(n, 100 * seed + i, values=(0, 1, 3, 300, 1000)), "gaps")
            xs = (lay, lay.sends(100 * seed + i))
        else:
            count = c if coll in (AG, BC, RD) else n * c + (3 if coll == AR else 0)
            xs = O.random_inputs(n, count, "f32", seed=5000 * (seed + 1) + i)
        calls.append((coll, sched, xs, inplace, root))
    assert len(calls) >= 18 and {c[0] for c in calls} == set(range(9)) and {c[1] for c in calls} == {G.RING, G.READ}
    assert {(c[0], c[1]) for c in calls} >= {(GA, G.RING), (GA, G.READ), (SC, G.RING), (SC, G.READ)}
    outs = G.run(n, calls, slice_bytes=256, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched, xs, _, root), out) in enumerate(zip(calls, outs)):
        _check(coll, xs, root, out, f"call {i} (coll {coll}, schedule {sched}, root {root})")


def test_sim_entry_points_keep_their_ranges(sim_lib):
    """The earlier entry points refuse collectives 7 and 8 as before; the new one takes them."""
    xs = G.gather_inputs(2, 16, 1)
    with pytest.raises(ValueError):
        G.V.run(2, [(GA, G.RING, [x.view(np.float32) for x in xs], False, 0)])
    with pytest.raises(ValueError):
        G.V.A.run(2, [(SC, G.RING, [x.view(np.float32) for x in xs], False, 0)])
    (out,) = G.run(2, [(GA, G.RING, xs, False, 1)])
    assert np.array_equal(out, G.gather_expect(xs))


# ---------------------------------------------------------------- kernel resources
def test_new_kernels_fit_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    ks = _kernels(tmp_path)
    for name in ("collect_push", "deal_push"):
        mine = {k: v for k, v in ks.items() if name in k}
        assert len(mine) == 6, (name, sorted(mine))  # 3 element sizes x (vector, scalar)
        for k, v in mine.items():
            assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
            assert v["private_segment_fixed_size"] == 0, (k, v)
        # the names stay out of the existing kernel-family count
        assert not [k for k in mine
                    if re.search(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push", k)]
