"""ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd without a GPU (-m "not gpu"): the ABI's checks
that need no communicator, the bookkeeping header (csrc/p2p.h) as a stand-alone program -- plain and
under the sanitizers -- the point-to-point geometry of csrc/schedule.h, the simulated kernel's protocol
and data (csrc/sim.cpp mnccl_sim_p2p: the kernel's wave-per-(pair, pipeline) mapping on the real slot /
flag / counter layout), and the new kernel's resource budget, read from the library.

The expected result of a transfer is its bytes: every send buffer holds seeded random bytes, every
recv buffer starts as fill bytes with 64 guard bytes behind it, and after a run a recv holds exactly
the bytes of the send it matches -- in call order per directed pair -- and its guard is unchanged.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sim_p2p_api as P
from test_kernel_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini-nccl_amd", "csrc")
FILL, GUARD = 0xA5, 64
# the simulator's geometry the issue sets: 2 slots, 2 pipelines, 1 KiB slots; every message may use both
SLOTS, C, SLOT, A = 2, 2, 1024, 2
SIZES = (700, SLOTS * A * SLOT, 3 * SLOTS * A * SLOT + 20)  # 1 slice; exactly slots x A; 3 x slots x A + 20 bytes
LARGEST = SIZES[-1]
SEEDS = [0, 1, 5]


# ---------------------------------------------------------------- the ABI, no communicator
def test_symbols_exported_and_bound(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    for f, nargs in (("ncclSend", 6), ("ncclRecv", 6), ("ncclGroupStart", 0), ("ncclGroupEnd", 0)):
        assert f in exported
        assert f in M.SIGNATURES and len(M.SIGNATURES[f][1]) == nargs
    assert all(callable(f) for f in (M.Comm.send, M.Comm.recv, M.group_start, M.group_end, M.group))
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version


def test_checks_before_the_communicator_is_read(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced on these paths
    for fn in (L.ncclSend, L.ncclRecv):
        # 1. a NULL comm; a NULL buffer with count != 0
        assert fn(fake, 4, M.ncclFloat, 0, None, None) == M.ncclInvalidArgument
        assert fn(fake, 0, M.ncclFloat, 0, None, None) == M.ncclInvalidArgument
        assert fn(fake, 4, M.ncclInt8, 0, None, None) == M.ncclInvalidArgument
        assert fn(None, 4, M.ncclFloat, 0, fake, None) == M.ncclInvalidArgument
        # 2. count == 0: success before the datatype is looked at or the communicator read
        assert fn(fake, 0, M.ncclFloat, 0, fake, None) == M.ncclSuccess
        assert fn(None, 0, M.ncclInt8, 99, fake, None) == M.ncclSuccess
        # 3. an unsupported datatype with count > 0: ncclInternalError, before the communicator is read
        for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
            assert fn(fake, 4, dt, 0, fake, None) == M.ncclInternalError


def test_group_calls_without_a_communicator(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)
    assert L.ncclGroupEnd() == M.ncclInvalidUsage  # no open group
    # nested Start / Start / End / End: success with nothing recorded; the group is then closed
    assert [L.ncclGroupStart(), L.ncclGroupStart(), L.ncclGroupEnd(), L.ncclGroupEnd()] == [0, 0, 0, 0]
    assert L.ncclGroupEnd() == M.ncclInvalidUsage
    # count == 0 inside a group records nothing (the fake communicator is never read at the end)
    assert L.ncclGroupStart() == 0
    assert L.ncclSend(fake, 0, M.ncclFloat, 1, fake, None) == M.ncclSuccess
    assert L.ncclRecv(fake, 0, M.ncclFloat, 1, fake, None) == M.ncclSuccess
    assert L.ncclGroupEnd() == M.ncclSuccess
    # a collective inside an open group: ncclInvalidUsage with nothing launched (the fake communicator
    # is never read), whichever of the seven; the group closes cleanly afterwards
    arr = (ctypes.c_size_t * 2)(4, 4)
    with M.group() as g:
        assert L.ncclAllReduce(fake, fake, 4, M.ncclFloat, M.ncclSum, fake, None) == M.ncclInvalidUsage
        assert L.ncclReduceScatter(fake, fake, 4, M.ncclFloat, M.ncclSum, fake, None) == M.ncclInvalidUsage
        assert L.ncclAllGather(fake, fake, 4, M.ncclFloat, fake, None) == M.ncclInvalidUsage
        assert L.ncclBroadcast(fake, fake, 4, M.ncclFloat, 0, fake, None) == M.ncclInvalidUsage
        assert L.ncclReduce(fake, fake, 4, M.ncclFloat, M.ncclSum, 0, fake, None) == M.ncclInvalidUsage
        assert L.ncclAllToAll(fake, fake, 4, M.ncclFloat, fake, None) == M.ncclInvalidUsage
        assert L.ncclAllToAllv(fake, arr, arr, fake, arr, arr, M.ncclFloat, fake, None) == M.ncclInvalidUsage
        # their own earlier checks still come first
        assert L.ncclAllReduce(fake, fake, 0, M.ncclFloat, M.ncclSum, fake, None) == M.ncclSuccess
        assert L.ncclAllReduce(None, fake, 4, M.ncclFloat, M.ncclSum, fake, None) == M.ncclInvalidArgument
    assert g.rc == M.ncclSuccess
    # with no group open a collective's checks are what they were
    assert L.ncclAllReduce(fake, fake, 4, M.ncclInt8, M.ncclSum, fake, None) == M.ncclInternalError
    # an argument error inside a group poisons it: ncclGroupEnd returns the first error, and the
    # thread's next group is clean
    assert L.ncclGroupStart() == 0
    assert L.ncclSend(fake, 4, M.ncclInt8, 0, fake, None) == M.ncclInternalError
    assert L.ncclRecv(None, 4, M.ncclFloat, 0, fake, None) == M.ncclInvalidArgument
    assert L.ncclGroupEnd() == M.ncclInternalError
    assert [L.ncclGroupStart(), L.ncclGroupEnd()] == [0, 0]
    assert L.ncclGroupEnd() == M.ncclInvalidUsage


def test_group_state_is_per_thread(nccl_lib):
    import threading
    import mini_nccl as M
    L, seen = nccl_lib, []
    assert L.ncclGroupStart() == 0
    t = threading.Thread(target=lambda: seen.append(L.ncclGroupEnd()))  # no group is open on THAT thread
    t.start()
    t.join()
    assert seen == [M.ncclInvalidUsage]
    assert L.ncclGroupEnd() == M.ncclSuccess


# ---------------------------------------------------------------- the bookkeeping header
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_bookkeeping_header_standalone(tmp_path, sanitize):
    """tests/native/p2p_selftest.cpp: csrc/p2p.h compiled into a stand-alone program (its own main, no
    HIP, nothing else linked) and run as a subprocess -- overlap detection, self pairing (equal,
    unequal, unpaired), per-pair ordering, kMaxGroupOps, the size_t overflow -- once plain and once with
    -fsanitize=address,undefined.  Nothing is loaded into Python."""
    exe = str(tmp_path / "p2p_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "p2p_selftest.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "p2p selftest: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


# ---------------------------------------------------------------- p2p_pipes and the slice map
CUS, WPS = 256, 2  # an MI355X's CUs; kernels.h kMinWavesPerSimd
PINNED_PIPES = {  # (n, C, most) -> p2p_pipes: the budget 256 x 4 x 2 / most over 2 (n - 1) pairs, clamped to [1, C]
    (2, 256, 1): 256, (2, 256, 8): 128, (2, 256, 16): 64, (3, 256, 1): 256, (3, 256, 8): 64, (3, 256, 16): 32,
    (8, 256, 1): 146, (8, 256, 8): 18, (8, 256, 16): 9, (16, 256, 1): 68, (16, 256, 8): 8, (16, 256, 16): 4,
}


@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("channels", [1, 2, 256])
@pytest.mark.parametrize("most", [1, 8, 16])
def test_p2p_pipes(sim_lib, n, channels, most):
    L = P.load()
    p = L.mnccl_p2p_pipes(n, channels, CUS, most, WPS)
    budget = L.mnccl_resident_cap(1, CUS, most, WPS)
    assert budget == CUS * 4 * WPS // most
    assert 1 <= p <= channels
    assert 2 * (n - 1) * p <= budget  # every directed pair's waves resident together
    assert p == min(channels, PINNED_PIPES[(n, 256, most)])
    # no rank enters the rule: whichever rank computes it gets this value (the function takes none),
    # and resident_pipes, which shares the budget helper, is what it was
    for P_ in (1, 64, 256, 512):
        for waves in (1, 4):
            cap = max(waves, CUS * 4 * WPS // most // waves * waves)
            assert L.mnccl_resident_cap(waves, CUS, most, WPS) == cap
            assert L.mnccl_resident_pipes(P_, waves, CUS, most, WPS) == min(P_, cap)


def test_group_capacity_constant(sim_lib):
    import p2p_workers
    assert P.load().mnccl_p2p_max_group_ops() == p2p_workers.MAX_GROUP_OPS == 64


def test_slice_map(sim_lib):
    """nslices = ceil(bytes / slot); A = min(p2p_pipes, nslices) pipelines; pipeline w carries slices
    w, w + A, ...: pinned for the simulator's geometry, and every slice on exactly one pipeline."""
    L = P.load()
    assert [L.mnccl_p2p_msg_pipes(b, SLOT, A) for b in SIZES] == [1, 2, 2]
    assert [[L.mnccl_p2p_pipe_msgs(b, SLOT, A, w) for w in range(C)] for b in SIZES] == [[1, 0], [2, 2], [7, 6]]
    for slot in (1024, 131072):
        for pipes in (1, 2, 3, 85, 256):
            for b in (1, 2, slot - 2, slot, slot + 2, 5 * slot, pipes * slot, pipes * slot + 2, 7 * pipes * slot + 20):
                ns = -(-b // slot)
                a = L.mnccl_p2p_msg_pipes(b, slot, pipes)
                assert a == min(pipes, ns)
                per = [L.mnccl_p2p_pipe_msgs(b, slot, pipes, w) for w in range(pipes)]
                assert per == [len(range(w, ns, a)) if w < a else 0 for w in range(pipes)] and sum(per) == ns


# ---------------------------------------------------------------- simulator
def _bytes(seed, *key, size):
    return np.frombuffer(np.random.default_rng([seed, *key]).bytes(size), np.uint8).copy()


def _recv(size):
    return np.full(size + GUARD, FILL, np.uint8)


def _ok(buf, want):
    return np.array_equal(buf[:want.size], want) and bool((buf[want.size:] == FILL).all())


def _pairs_consistent(tx, rx):
    n = tx.shape[0]
    return all(np.array_equal(tx[r][q], rx[q][r]) for r in range(n) for q in range(n) if q != r)


def _run(n, phases, seed, **kw):
    return P.run(n, phases, channels=C, slots=SLOTS, slot_bytes=SLOT, pipes=A, seed=seed, **kw)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", SIZES)
def test_sim_a_two_ranks(sim_lib, size, seed):
    """(a) n = 2: an ungrouped send met by an ungrouped recv, then a grouped exchange both ways, at one
    slice, at exactly slots x A slices and at 3 x slots x A slices + 20 bytes."""
    L = P.load()
    x01, x10, y01 = _bytes(seed, 0, 1, size=size), _bytes(seed, 1, 0, size=size), _bytes(seed, 2, size=size)
    r0, r1, q1 = _recv(size), _recv(size), _recv(size)
    one_way = {0: [[("send", 1, y01)]], 1: [[("recv", 0, q1[:size])]]}
    both = {0: [[("send", 1, x01), ("recv", 1, r0[:size])]], 1: [[("recv", 0, r1[:size]), ("send", 0, x10)]]}
    _, tx, rx = _run(2, [one_way, both], seed)
    assert _ok(q1, y01) and _ok(r1, x01) and _ok(r0, x10)
    per = [L.mnccl_p2p_pipe_msgs(size, SLOT, A, w) for w in range(C)]
    assert list(tx[0][1]) == [2 * m for m in per] and list(rx[1][0]) == [2 * m for m in per]
    assert list(tx[1][0]) == per and list(rx[0][1]) == per


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("order", ["recv_send", "send_recv"])
def test_sim_b_asymmetric_grouping(sim_lib, order, seed):
    """(b) rank 0 calls group{send -> 1, recv <- 1} while rank 1 calls recv <- 0 and send -> 0
    ungrouped, in either order, at the largest size (the message outgrows the slots three times
    over): no deadlock and the right bytes, because no wave serves two pairs."""
    x01, x10 = _bytes(seed, 0, 1, size=LARGEST), _bytes(seed, 1, 0, size=LARGEST)
    r0, r1 = _recv(LARGEST), _recv(LARGEST)
    mine = [[("recv", 0, r1[:LARGEST])], [("send", 0, x10)]]
    phase = {0: [[("send", 1, x01), ("recv", 1, r0[:LARGEST])]], 1: mine if order == "recv_send" else mine[::-1]}
    _, tx, rx = _run(2, [phase], seed)
    assert _ok(r1, x01) and _ok(r0, x10) and _pairs_consistent(tx, rx)


def test_sim_b_the_deadlock_the_rule_names(sim_lib):
    """The header's deadlock rule, seen by the simulator: both ranks send and then receive, ungrouped,
    with a message larger than the pair's slots -- no progress.  At one slice the sends fit the slots
    and complete early (which the header allows but does not promise)."""
    def phase(size):
        xs = [_bytes(9, r, size=size) for r in range(2)]
        rs = [_recv(size) for _ in range(2)]
        return {r: [[("send", 1 - r, xs[r])], [("recv", 1 - r, rs[r][:size])]] for r in range(2)}, xs, rs
    with pytest.raises(RuntimeError):
        _run(2, [phase(LARGEST)[0]], 0)
    ph, xs, rs = phase(SIZES[0])
    _run(2, [ph], 0)
    assert _ok(rs[0], xs[1]) and _ok(rs[1], xs[0])


@pytest.mark.parametrize("seed", SEEDS)
def test_sim_c_all_pairs(sim_lib, seed):
    """(c) n = 4, one group per rank with a send to and a recv from every rank, itself included; a
    different count per pair, zeros among them."""
    n = 4
    sizes = [[(0, 700, LARGEST, 20, 4096, 1026, 2)[(3 * r + 2 * q + seed) % 7] for q in range(n)] for r in range(n)]
    assert any(sizes[r][q] == 0 for r in range(n) for q in range(n))
    xs = [[_bytes(seed, r, q, size=sizes[r][q]) for q in range(n)] for r in range(n)]
    rs = [[_recv(sizes[q][r]) for q in range(n)] for r in range(n)]  # rs[r][q]: what r receives from q
    phase = {r: [[("send", q, xs[r][q]) for q in range(n)] + [("recv", q, rs[r][q][:sizes[q][r]]) for q in range(n)]]
             for r in range(n)}
    _, tx, rx = _run(n, [phase], seed)
    for r in range(n):
        for q in range(n):
            assert _ok(rs[r][q], xs[q][r]), (r, q)
    assert _pairs_consistent(tx, rx)
    L = P.load()
    for r in range(n):
        for q in range(n):
            want = [L.mnccl_p2p_pipe_msgs(sizes[r][q], SLOT, A, w) if q != r else 0 for w in range(C)]
            assert list(tx[r][q]) == want, (r, q)


@pytest.mark.parametrize("seed", SEEDS)
def test_sim_d_two_sends_in_order(sim_lib, seed):
    """(d) two sends of different sizes to one peer in one group, matched by two separate ungrouped
    recvs -- and two ungrouped sends matched by one group of two recvs: call order per pair."""
    big, small = LARGEST, 700
    for first, second in ((big, small), (small, big)):
        a, b = _bytes(seed, 1, size=first), _bytes(seed, 2, size=second)
        ra, rb = _recv(first), _recv(second)
        grouped = {0: [[("send", 1, a), ("send", 1, b)]], 1: [[("recv", 0, ra[:first])], [("recv", 0, rb[:second])]]}
        _, tx, rx = _run(2, [grouped], seed)
        assert _ok(ra, a) and _ok(rb, b) and _pairs_consistent(tx, rx)
        ra, rb = _recv(first), _recv(second)
        reverse = {0: [[("send", 1, a)], [("send", 1, b)]], 1: [[("recv", 0, ra[:first]), ("recv", 0, rb[:second])]]}
        _, tx, rx = _run(2, [reverse], seed)
        assert _ok(ra, a) and _ok(rb, b) and _pairs_consistent(tx, rx)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("sched", [P.RING, P.READ], ids=["ring", "read"])
def test_sim_e_interleaved_with_an_allreduce(sim_lib, sched, seed):
    """(e) a ring shift by send / recv, an all-reduce, the ring shift again, on one state: the counters
    every schedule shares stay consistent pair by pair and every result is right.  (Integer-valued
    fp32 inputs: their sum is exact in any order.)"""
    n, size = 3, LARGEST

    def shift(tag):
        xs = [_bytes(seed, tag, r, size=size) for r in range(n)]
        rs = [_recv(size) for _ in range(n)]
        return {r: [[("send", (r + 1) % n, xs[r]), ("recv", (r - 1) % n, rs[r][:size])]] for r in range(n)}, xs, rs
    s1, x1, r1 = shift(1)
    s2, x2, r2 = shift(2)
    g = np.random.default_rng(seed)
    ins = [g.integers(-1000, 1000, n * 1100).astype(np.float32) for _ in range(n)]
    outs, tx, rx = _run(n, [s1, ("ar", sched, ins), s2], seed)
    for r in range(n):
        assert _ok(r1[r], x1[(r - 1) % n]) and _ok(r2[r], x2[(r - 1) % n]), r
        assert np.array_equal(outs[1][r], sum(ins)), r
    assert _pairs_consistent(tx, rx)
    L = P.load()
    per = np.array([L.mnccl_p2p_pipe_msgs(size, SLOT, A, w) for w in range(C)], dtype=np.uint64)
    # the counters are the all-reduce's own (the same call alone on a fresh state) plus the two shifts'
    _, tx0, rx0 = _run(n, [("ar", sched, ins)], seed)
    for r in range(n):
        tx0[r][(r + 1) % n] += 2 * per
        rx0[r][(r - 1) % n] += 2 * per
    assert np.array_equal(tx, tx0) and np.array_equal(rx, rx0)


@pytest.mark.parametrize("seed", SEEDS)
def test_sim_f_the_same_group_three_times(sim_lib, seed):
    """(f) the same group run three times on one state (what a graph replay does): new bytes every
    time, the counters three times one run's."""
    n, size = 2, LARGEST
    phases, xs, rs = [], [], []
    for k in range(3):
        xs.append([_bytes(seed, k, r, size=size) for r in range(n)])
        rs.append([_recv(size) for _ in range(n)])
        phases.append({r: [[("send", 1 - r, xs[k][r]), ("recv", 1 - r, rs[k][r][:size])]] for r in range(n)})
    _, tx, rx = _run(n, phases, seed)
    for k in range(3):
        assert _ok(rs[k][0], xs[k][1]) and _ok(rs[k][1], xs[k][0]), k
    L = P.load()
    assert list(tx[0][1]) == [3 * L.mnccl_p2p_pipe_msgs(size, SLOT, A, w) for w in range(C)]
    assert _pairs_consistent(tx, rx)


def test_sim_refuses_what_the_header_refuses(sim_lib):
    x, r = _bytes(1, size=64), _recv(64)
    with pytest.raises(ValueError):  # an unpaired self send
        _run(2, [{0: [[("send", 0, x)]]}], 0)
    with pytest.raises(ValueError):  # a recv over a send of the same group
        _run(2, [{0: [[("send", 1, x), ("recv", 1, x[:32])]], 1: [[("recv", 0, r[:64]), ("send", 0, x[:32])]]}], 0)


# ---------------------------------------------------------------- kernel resources
def test_p2p_kernel_fits_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    all_ks = _kernels(tmp_path)
    ks = {k: v for k, v in all_ks.items() if "p2p_kernel" in k}
    assert len(ks) == 1, sorted(ks)  # one kernel: each end's path is chosen per operation at run time
    for k, v in ks.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the existing counts are what they were, and the new name stays out of them
    old = re.compile(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push")
    assert not [k for k in ks if old.search(k)]
    assert len([k for k in all_ks if old.search(k)]) == 5 * 40 + 3 * 6
    assert len([k for k in all_ks if "varblock_push" in k]) == 3
