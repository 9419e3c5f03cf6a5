"""ncclAllToAllv without a GPU (-m "not gpu"): the ABI's argument checks, the host-side rules
(csrc/varblock.h) on hand-made cases, the simulated kernel's protocol and data on both schedules --
alone and mixed with the six other collectives on one communicator state -- the host code under the
sanitizers as a stand-alone program, and the new kernel's resource budget, read from the library.

The expected result is the permutation itself, computed with numpy slicing
(sim_alltoallv_api.Layout.expect): elements [sdispls[q], +C[r][q]) of rank r's send are elements
[rdispls[r], +C[r][q]) of rank q's recv.  Buffers are seeded random BYTES, different per rank and
call, compared as bytes; a recv starts as fill bytes, so the gaps between its blocks must come back
unchanged, as must the 256 guard bytes behind it and the send (sim_alltoallv_api.run).
"""
import ctypes
import os
import re
import shutil
import socket
import subprocess

import numpy as np
import pytest

import sim_alltoall_api as A
import sim_alltoallv_api as V
from test_kernel_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini-nccl_amd", "csrc")
AR, RS, AG, BC, RD, A2A, A2AV = range(7)
DEFAULT_SLICE = 128 << 10  # MINI_NCCL_SLICE_SIZE's default
MODES = ("contig", "reversed", "gaps")


# ---------------------------------------------------------------- the ABI
def test_symbol_exported_and_bound(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    assert "ncclAllToAllv" in exported
    assert "ncclAllToAllv" in M.SIGNATURES and len(M.SIGNATURES["ncclAllToAllv"][1]) == 9
    assert callable(M.Comm.all_to_all_v)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version


def test_argument_checks_before_the_communicator_is_read(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)  # never dereferenced on these paths
    arr = (ctypes.c_size_t * 2)(4, 4)
    call = lambda comm, sc=arr, sd=arr, rc=arr, rd=arr, dt=M.ncclFloat, s=fake, r=other: \
        L.ncclAllToAllv(s, sc, sd, r, rc, rd, dt, comm, None)
    # 1. a NULL comm or a NULL array, before the datatype
    assert call(None) == M.ncclInvalidArgument
    assert call(None, dt=M.ncclInt8) == M.ncclInvalidArgument
    for k in ("sc", "sd", "rc", "rd"):
        assert call(fake, **{k: None}) == M.ncclInvalidArgument
        assert call(fake, dt=M.ncclInt8, **{k: None}) == M.ncclInvalidArgument
    # 2. an unsupported datatype: ncclInternalError, before the communicator (a fake pointer) is read
    #    -- and before the buffers are looked at (NULL buffers are the communicator's business)
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert call(fake, dt=dt) == M.ncclInternalError
        assert call(fake, dt=dt, s=None, r=None) == M.ncclInternalError


# ---------------------------------------------------------------- the host-side rules
def test_local_checks(sim_lib):
    s, r = 0x10000, 0x80000
    c, d, z = [4, 0, 7], [0, 4, 4], [0, 0, 0]
    assert V.check_local(4, s, c, d, r, c, d) == 0
    # NULL buffers: fine with all-zero counts on that side (an idle rank), refused otherwise
    assert V.check_local(4, None, z, z, None, z, z) == 0
    assert V.check_local(4, None, z, d, r, c, d) == 0
    assert V.check_local(4, s, c, d, None, z, d) == 0
    assert V.check_local(4, None, c, d, r, c, d) == 1
    assert V.check_local(4, s, c, d, None, [0, 0, 1], d) == 1
    # overflow: displ + count, the byte size, the address
    top = (1 << 64) - 1
    assert V.check_local(4, s, c, [top - 2, 0, 4], r, c, d) == 2
    assert V.check_local(4, s, [top // 4 + 1, 0, 0], z, r, c, d) == 2
    assert V.check_local(8, s, c, d, top - 15, [2, 0, 0], z) == 2
    assert V.check_local(4, s, c, d, r, c, [top, 0, 4]) == 2
    assert V.check_local(4, s, [0, 0, 0], [top, top, top], r, z, [top, top, top]) == 0  # empty blocks' displs unused
    # overlapping recv blocks (the last element of block 0 is the first of block 2) -- and the same
    # displacements on the send side are accepted: send blocks are only read
    assert V.check_local(4, s, c, d, r, c, [0, 4, 3]) == 3
    assert V.check_local(4, s, c, [0, 4, 3], r, c, d) == 0
    assert V.check_local(4, s, c, [0, 0, 0], r, c, d) == 0
    assert V.check_local(4, s, c, d, r, c, [0, 1, 4]) == 0  # an empty block inside another overlaps nothing
    # recv overlapping send: partly, wholly, by one byte -- but not when merely adjacent
    assert V.check_local(4, s, c, d, s, c, d) == 4
    assert V.check_local(4, s, c, d, s + 40, c, d) == 4
    assert V.check_local(4, s, c, d, s + 43, c, d) == 4
    assert V.check_local(4, s, c, d, s + 44, c, d) == 0
    assert V.check_local(2, s + 1, c, d, s + 23, c, d) == 0  # odd addresses, adjacent
    assert V.check_local(4, s, c, d, s + 16, [0, 0, 0], z) == 0  # nothing is received: nothing overlaps


def test_matrix_check(sim_lib):
    for n in (1, 2, 5, 16):
        C = V.random_matrix(n, 3)
        assert V.matrix_mismatch(C, C.T) == 0
        for r, q in ((0, 0), (n - 1, 0), (n // 2, n - 1)):
            bad = C.T.copy()
            bad[q, r] += 1  # rank q expects one element more from rank r
            assert V.matrix_mismatch(C, bad) == 1 + r * n + q
    assert V.matrix_mismatch([[0, 1], [0, 0]], [[0, 0], [0, 0]]) == 2  # rank 0 sends one element nobody expects


def test_slice_length_rule(sim_lib):
    L = V.load()
    for bytes_, slice_ in ((0, 16), (1, 16), (16, 16), (17, 16), (65644, 1024), (6, 1024)):
        lens = [L.mnccl_varblock_len(bytes_, slice_, s) for s in range(bytes_ // slice_ + 3)]
        assert sum(lens) == bytes_ and all(0 <= x <= slice_ for x in lens)
        assert lens == sorted(lens, reverse=True)  # full slices, one short one, then zeros for good


# ---------------------------------------------------------------- simulator
NS_SIM = [1, 2, 3, 4, 5, 8, 9, 16]


def _exact(n, lay, sched, slice_bytes, channels, seed, calls=1, min_slice=0):
    sends = [lay.sends(1000 * seed + i) for i in range(calls)]
    outs = V.run(n, [(A2AV, sched, (lay, s), False, 0) for s in sends], esz=lay.esz, slice_bytes=slice_bytes,
                 channels=channels, seed=seed, min_slice=min_slice)
    for i, (s, out) in enumerate(zip(sends, outs)):
        for q, e in enumerate(lay.expect(s)):
            assert np.array_equal(out[q], e), f"n={n} sched={sched} mode={lay.mode} slice={slice_bytes} C={channels} " \
                                              f"seed={seed} call {i}: rank {q} differs (blocks or gaps)"


def _special(n, kind):
    C = np.zeros((n, n), dtype=np.int64)
    if kind == "one_large":
        C[n - 1, 0] = 16411  # the last rank's block for rank 0 (n = 1: the own block)
    elif kind == "zero_row_col":
        C = V.random_matrix(n, 77)
        C[n // 2, :] = 0
        C[:, n // 2] = 0
    return C


@pytest.mark.parametrize("sched", [V.RING, V.READ], ids=["ring", "read"])
@pytest.mark.parametrize("n", NS_SIM)
def test_sim_alltoallv(sim_lib, n, sched):
    """Seeded random matrices with entries from {0, 1, 3, 300, 16411} x slices of 16 B, 1 KiB and the
    default x displacements contiguous, reversed and with 3-element gaps, channels 1 and 4 alternating
    with the scheduling seed; a second call on the same state for every third seed.  Then an all-zero
    matrix, an all-zero row and column, and one large block among empty ones.  Exact, no deadlock."""
    seed = 0
    for slice_bytes in (16, 1024, DEFAULT_SLICE):
        for mode in MODES:
            # (16-byte slices of 16411-element blocks: ~4100 slices; a few seeds suffice at size)
            for _ in range(2 if slice_bytes == 16 and n > 5 else 4):
                seed += 1
                values = (0, 1, 3, 300) if slice_bytes == 16 and n > 8 else (0, 1, 3, 300, 16411)
                lay = V.Layout(V.random_matrix(n, seed, values), mode, esz=(4, 2)[seed % 2])
                _exact(n, lay, sched, slice_bytes, (1, 4)[seed % 2], seed % 5, calls=2 if seed % 3 == 0 else 1)
    for kind in ("zeros", "zero_row_col", "one_large"):
        for mode in MODES:
            seed += 1
            _exact(n, V.Layout(_special(n, kind), mode), sched, (16, 1024)[seed % 2], (1, 4)[seed % 2], seed, calls=2)
    # the adaptive slice of Comm::make_params (min_slice != 0), as the library picks it
    _exact(n, V.Layout(V.random_matrix(n, 99), "gaps"), sched, DEFAULT_SLICE, 4, 3, calls=2, min_slice=1024)


def test_uniform_counts_give_alltoall_exactly(sim_lib):
    """Uniform counts with contiguous displacements: the v form's recv is ncclAllToAll's, byte for byte."""
    for n in (2, 3, 8):
        for count in (1, 300, 4099):
            for sched in (V.RING, V.READ):
                xs = A.random_blocks(n, 4 * count, 5 * n + count)
                (plain,) = A.run(n, [(A2A, sched, xs, False, 0)], slice_bytes=1024, channels=4, seed=2)
                lay = V.Layout(np.full((n, n), count), "contig")
                (var,) = V.run(n, [(A2AV, sched, (lay, xs), False, 0)], slice_bytes=1024, channels=4, seed=2)
                assert all(np.array_equal(a, b) for a, b in zip(plain, var)), (n, count, sched)


@pytest.mark.parametrize("seed", [0, 1, 7, 12])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (4, 4), (5, 1), (8, 8), (9, 4), (16, 2)])
def test_sim_mixed_sequence_of_all_seven(sim_lib, oracle_lib, n, channels, seed):
    """16 calls on one communicator state mixing all seven collectives and both schedules: the first
    seven are one of each, every other call after that is a variable all-to-all.  Every call exact:
    the counters the schedules share stay in step."""
    import oracle_api as O
    from test_alltoall_cpu import _check as check_other
    g = np.random.default_rng(9000 * n + seed)
    sizes = (4099, 1, 1000, 256, 255, 700, 3)
    calls = []
    for i in range(16):
        coll = (i + seed) % 7 if i < 7 else A2AV if i % 2 else int(g.integers(0, 7))
        sched = int(g.choice([V.RING, V.READ]))
        root = int(g.integers(0, n))
        c = int(sizes[int(g.integers(0, len(sizes)))])
        if coll == A2AV:
            lay = V.Layout(V.random_matrix(n, 100 * seed + i, (0, 1, 3, 300, 4099)), MODES[i % 3])
            xs = (lay, lay.sends(100 * seed + i))
        elif coll == A2A:
            xs = A.random_blocks(n, 4 * c, 100 * seed + i)
        else:
            count = c if coll in (AG, BC, RD) else n * c + (3 if coll == AR else 0)
            xs = O.random_inputs(n, count, "f32", seed=5000 * (seed + 1) + i)
        calls.append((coll, sched, xs, False, root))
    assert {c[0] for c in calls} == set(range(7)) and {c[1] for c in calls} == {V.RING, V.READ}
    outs = V.run(n, calls, slice_bytes=256, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched, xs, _, root), out) in enumerate(zip(calls, outs)):
        what = f"call {i} (coll {coll}, schedule {sched}, root {root})"
        if coll == A2AV:
            for q, e in enumerate(xs[0].expect(xs[1])):
                assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
        else:
            check_other(coll, xs, root, out, what)


def test_existing_entry_points_keep_their_ranges(sim_lib):
    """mnccl_sim_mixed refuses collective 6 as it refused everything past 5; mnccl_sim_varblock takes it."""
    lay = V.Layout([[1, 2], [3, 4]])
    xs = lay.sends(1)
    with pytest.raises(ValueError):
        A.run(2, [(A2AV, V.RING, [np.zeros(16, np.uint8)] * 2, False, 0)])
    (out,) = V.run(2, [(A2AV, V.RING, (lay, xs), False, 0)])
    assert all(np.array_equal(o, e) for o, e in zip(out, lay.expect(xs)))


# ---------------------------------------------------------------- host code under sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_code_under_asan_ubsan(tmp_path):
    """tests/native/alltoallv_selftest.cpp: a stand-alone program (its own main) compiled together
    with csrc/sim.cpp and the host sources it links, -fsanitize=address,undefined, run as a
    subprocess: the simulator in miniature, the rules, and the board's rendezvous with rows on rank
    threads.  Nothing is loaded into Python."""
    exe = str(tmp_path / "alltoallv_selftest")
    srcs = [os.path.join(ROOT, "tests", "native", "alltoallv_selftest.cpp")] + \
        [os.path.join(CSRC, f) for f in ("sim.cpp", "bootstrap.cpp", "config.cpp", "peerbuf.cpp", "ipcreg.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + CSRC, "-o", exe] + srcs + ["-L/opt/rocm/lib", "-lamdhip64", "-lhsa-runtime64", "-lrt", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINI_NCCL_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(port)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "alltoallv selftest: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


# ---------------------------------------------------------------- kernel resources
def test_varblock_push_fits_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    all_ks = _kernels(tmp_path)
    ks = {k: v for k, v in all_ks.items() if "varblock_push" in k}
    assert len(ks) == 3, sorted(ks)  # by element size only: 2, 4, 8 (the path is chosen per destination at run time)
    for k, v in ks.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the existing counts are what they were, and the new name stays out of them
    old = re.compile(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push")
    assert not [k for k in ks if old.search(k)]
    assert len([k for k in all_ks if old.search(k)]) == 5 * 40 + 3 * 6
    assert len([k for k in all_ks if "exchange_push" in k]) == 6
