"""ncclAllToAll without a GPU (-m "not gpu"): the ABI's argument checks, the ring's hop table
(csrc/schedule.h coll_op), the simulated kernels' protocol and data on both schedules -- alone and
mixed with the five other collectives on one communicator state -- the simulator under the host
sanitizers as a stand-alone program, and the new kernel's resource budget, read from the library.

The expected result is the permutation itself (sim_alltoall_api.expect): block r of rank q's recv is
block q of rank r's send.  Buffers are seeded random BYTES, different per rank and call, compared as
bytes; after every call the 256 guard bytes past each recv and the send must be unchanged
(sim_alltoall_api.run).

The ring and one slot: a kForward op receives message m and sends m + 1, and with one slot per
pipeline its send waits for the credit the next rank only returns inside its own op of the same
index -- the cycle test_schedule.py::test_single_slot_fifo_deadlocks pins for the all-reduce, and
why Config clamps MINI_NCCL_SLOTS to >= 2.  The all-to-all's table has kForward ops from 3 ranks
on, so slots = 1 runs on the read schedule at every rank count (it uses no slots) and on the ring
where the table has no kForward (n <= 2); test_ring_with_one_slot_is_refused_by_the_protocol pins
the rest.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sim_alltoall_api as A
from test_kernel_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini-nccl_amd", "csrc")
AR, RS, AG, BC, RD, A2A = range(6)
K_SEND, K_COPY, K_FORWARD = 0, 4, 5
DEFAULT_SLICE = 128 << 10  # MINI_NCCL_SLICE_SIZE's default


# ---------------------------------------------------------------- the ABI
def test_symbol_exported_and_bound(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    assert "ncclAllToAll" in exported
    assert "ncclAllToAll" in M.SIGNATURES and len(M.SIGNATURES["ncclAllToAll"][1]) == 6
    assert callable(M.Comm.all_to_all)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version


def test_argument_checks_before_device_work(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)  # never dereferenced on these paths
    a2a = lambda s, r, c, dt, comm: L.ncclAllToAll(s, r, c, dt, comm, None)
    # 1. NULL comm / sendbuff / recvbuff, before anything else
    assert a2a(fake, other, 4, M.ncclFloat, None) == M.ncclInvalidArgument
    assert a2a(None, other, 4, M.ncclFloat, fake) == M.ncclInvalidArgument
    assert a2a(fake, None, 4, M.ncclFloat, fake) == M.ncclInvalidArgument
    assert a2a(None, other, 0, M.ncclInt8, fake) == M.ncclInvalidArgument
    assert a2a(fake, other, 0, M.ncclFloat, None) == M.ncclInvalidArgument
    # 2. count == 0 -> success before the datatype (or the communicator) is looked at
    assert a2a(fake, other, 0, M.ncclInt8, fake) == M.ncclSuccess
    assert a2a(fake, fake, 0, M.ncclFloat, fake) == M.ncclSuccess
    # 3. unsupported datatype -> ncclInternalError, before the communicator is touched (the overlap
    #    rule comes after it: send == recv here)
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert a2a(fake, other, 4, dt, fake) == M.ncclInternalError
        assert a2a(fake, fake, 4, dt, fake) == M.ncclInternalError


# ---------------------------------------------------------------- op table
NS_TABLE = [2, 3, 4, 5, 6, 7, 8, 9, 16]


@pytest.mark.parametrize("n", NS_TABLE)
def test_op_table_counts_and_messages(sim_lib, n):
    S = A.R.S
    A.load()
    nops, msgs = S.num_ops(A2A, n), S.msgs_per_iter(A2A, n)
    assert nops == (n - 1) * (n + 2) // 2
    assert msgs == n * (n - 1) // 2
    tables = [[A.R.coll_op(A2A, n, r, k, 0) for k in range(nops)] for r in range(n)]
    for r in range(n):
        assert A.R.tx_msgs(A2A, n, r, 0) == A.R.rx_msgs(A2A, n, r, 0) == msgs
        assert [S.coll_op(A2A, n, r, k) for k in range(nops)] == tables[r]  # the rootless export answers too
        assert A.R.coll_op(A2A, n, r, nops - 1, n - 1) == tables[r][nops - 1]  # no root dependence
        sends = [o[2] for o in tables[r] if o[2] >= 0]
        recvs = [o[3] for o in tables[(r + 1) % n] if o[3] >= 0]
        assert sends == recvs == list(range(msgs))  # rank r's send sequence is rank r+1's receive sequence
        # the table's order: for d = 1 .. n-1, a kSend, d - 1 kForwards, a kCopy
        k = 0
        for d in range(1, n):
            m = d * (d - 1) // 2
            assert tables[r][k] == (K_SEND, (r + d) % n, m, -1)
            for j in range(1, d):
                kind, _, send_msg, recv_msg = tables[r][k + j]
                assert (kind, send_msg, recv_msg) == (K_FORWARD, m + j, m + j - 1)
            assert tables[r][k + d] == (K_COPY, (r - d) % n, -1, m + d - 1)
            k += d + 1
        assert k == nops


@pytest.mark.parametrize("n", NS_TABLE)
def test_op_table_delivers_every_pair_once(sim_lib, n):
    """Follow every message hop by hop: rank s's kSend of send block d, message m, is received by
    the op of rank s + 1 whose recv_msg is m; a kForward hands it on under its send_msg; a kCopy ends
    it in a recv block.  Every ordered pair (s, d), s != d, must arrive exactly once, in recv block
    s of rank d, from send block d of rank s."""
    S = A.R.S
    nops = S.num_ops(A2A, n)
    tables = [[S.coll_op(A2A, n, r, k) for k in range(nops)] for r in range(n)]
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
            assert block != s and at == block, (n, s, block, at)  # send block d reaches rank d
            assert o[1] == s, (n, s, block, o)                    # into recv block s
            assert (s, at) not in delivered
            delivered[(s, at)] = hops
    assert set(delivered) == {(s, d) for s in range(n) for d in range(n) if s != d}
    assert all(h == (d - s) % n for (s, d), h in delivered.items())  # the block for s + d travels d hops


# ---------------------------------------------------------------- simulator
NS_SIM = [1, 2, 3, 4, 5, 8, 9, 16]
SEEDS = 20


def _one(n, sched, count, slice_bytes, channels, slots, seed, calls=2):
    """`calls` all-to-alls in a row on one state (fresh bytes each): a call whose counters ended out
    of step with its peers' deadlocks or corrupts the next."""
    sends = [A.random_blocks(n, 4 * count, 1000 * seed + i) for i in range(calls)]
    outs = A.run(n, [(A2A, sched, xs, False, 0) for xs in sends], slice_bytes=slice_bytes, channels=channels, slots=slots,
                 seed=seed)
    for i, (xs, out) in enumerate(zip(sends, outs)):
        for q, e in enumerate(A.expect(xs)):
            assert np.array_equal(out[q], e), f"n={n} sched={sched} count={count} slice={slice_bytes} C={channels} " \
                                              f"K={slots} seed={seed} call {i}: rank {q} differs"


@pytest.mark.parametrize("sched", [A.RING, A.READ], ids=["ring", "read"])
@pytest.mark.parametrize("n", NS_SIM)
def test_sim_alltoall(sim_lib, n, sched):
    """Slices of 16 B, 1 KiB and the default x counts 1, 3, 300 and 16411 per block, 20 schedule
    seeds each (seed 0 is the round-robin order), channels 1 and 4 and slots 1 and 2 alternating
    with the seed so every pair of them meets every (slice, count).  Exact, no deadlock, and -- for
    every fifth seed -- a second call on the same state exact too: counters in step.  (The ring with
    one slot: the module docstring.)"""
    one_slot_ok = sched == A.READ or n <= 2
    for slice_bytes in (16, 1024, DEFAULT_SLICE):
        for count in (1, 3, 300, 16411):
            # (4103 16-byte slices of 16 ranks' (n-1)(n+2)/2-op table: a second call adds nothing there)
            heavy = slice_bytes == 16 and count == 16411 and n > 5
            for seed in range(SEEDS):
                calls = 2 if seed % 5 == 0 and not heavy else 1
                channels = (1, 4)[seed % 2]
                slots = (1, 2)[(seed // 2) % 2] if one_slot_ok else 2
                _one(n, sched, count, slice_bytes, channels, slots, seed, calls)


@pytest.mark.parametrize("n", [3, 4, 5, 8, 9, 16])
def test_ring_with_one_slot_is_refused_by_the_protocol(sim_lib, n):
    # the kForward cycle of the module docstring; Config never lets a communicator have one slot
    with pytest.raises(RuntimeError, match="deadlock"):
        _one(n, A.RING, 300, 64, 2, 1, 0, calls=1)


def _check(coll, xs, root, out, what):
    from test_rooted_cpu import _check as check_other
    if coll == A2A:
        for q, e in enumerate(A.expect(xs)):
            assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
    else:
        check_other(coll, xs, root, out, [None] * len(xs), what)


@pytest.mark.parametrize("seed", [0, 1, 7, 12])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (4, 4), (5, 1), (8, 8), (9, 4), (16, 2)])
def test_sim_mixed_sequence_on_one_state(sim_lib, oracle_lib, n, channels, seed):
    """14 calls on one communicator state mixing all six collectives and both schedules: the first
    six are one of each, every other call is an all-to-all or random.  Every call exact."""
    import oracle_api as O
    g = np.random.default_rng(7000 * n + seed)
    sizes = (4099, 1, 1000, 256, 255, 700, 3)
    calls = []
    for i in range(14):
        coll = (i + seed) % 6 if i < 6 else A2A if i % 2 else int(g.integers(0, 6))
        sched = int(g.choice([A.RING, A.READ]))
        root = int(g.integers(0, n))
        c = int(sizes[int(g.integers(0, len(sizes)))])
        if coll == A2A:
            xs = A.random_blocks(n, 4 * c, 100 * seed + i)
        else:
            count = c if coll in (AG, BC, RD) else n * c + (3 if coll == AR else 0)
            xs = O.random_inputs(n, count, "f32", seed=5000 * (seed + 1) + i)
        calls.append((coll, sched, xs, False, root))
    assert {c[0] for c in calls} == set(range(6)) and {c[1] for c in calls} == {A.RING, A.READ}
    outs = A.run(n, calls, slice_bytes=256, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched, xs, _, root), out) in enumerate(zip(calls, outs)):
        _check(coll, xs, root, out, f"call {i} (coll {coll}, schedule {sched}, root {root})")


def test_sim_entry_points_keep_their_ranges(sim_lib):
    """mnccl_sim_collective and mnccl_sim_rooted refuse collective 5 as before; mnccl_sim_mixed takes it."""
    xs = A.random_blocks(2, 16, 1)
    with pytest.raises(ValueError):
        A.R.run(2, [(A2A, A.RING, [x.view(np.float32) for x in xs], False, 0)])
    with pytest.raises(ValueError):
        A.R.S.run(2, [(A2A, A.RING, [x.view(np.float32) for x in xs], False)])
    (out,) = A.run(2, [(A2A, A.RING, xs, False, 0)])
    assert all(np.array_equal(o, e) for o, e in zip(out, A.expect(xs)))


# ---------------------------------------------------------------- host code under sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_simulator_under_asan_ubsan(tmp_path):
    """tests/native/alltoall_selftest.cpp: a stand-alone program (its own main) compiled together
    with csrc/sim.cpp and the host sources it links, -fsanitize=address,undefined, run as a
    subprocess.  Nothing is loaded into Python."""
    exe = str(tmp_path / "alltoall_selftest")
    srcs = [os.path.join(ROOT, "tests", "native", "alltoall_selftest.cpp")] + \
        [os.path.join(CSRC, f) for f in ("sim.cpp", "bootstrap.cpp", "config.cpp", "peerbuf.cpp", "ipcreg.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + CSRC, "-o", exe] + srcs + ["-L/opt/rocm/lib", "-lamdhip64", "-lhsa-runtime64", "-lrt", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINI_NCCL_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "alltoall selftest: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


# ---------------------------------------------------------------- kernel resources
def test_exchange_push_fits_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if "exchange_push" in k}
    assert len(ks) == 6, sorted(ks)  # 3 element sizes x (vector, scalar)
    for k, v in ks.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the name stays out of the existing 120-kernel count
    assert not [k for k in ks if re.search(r"(ring|read|oneshot)_kernel", k)]
