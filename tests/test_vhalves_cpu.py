"""mncclAllGatherv / mncclReduceScatterv without a GPU (-m "not gpu"): the ABI's argument checks in
their order, the host-side rules (csrc/vhalves.h) on hand-made cases, the length rule against a numpy
restatement, the simulated kernels' protocol and data on both schedules -- alone and interleaved with
the other collectives on one communicator state -- and the new kernels' resource budget, read from
the library.

Expected results are exact: the gather is the permutation itself on seeded random bytes
(sim_vhalves_api.Shape.gather_expect); the fold is oracle_api.ring_fold on block c laid into chunk c
(Shape.fold_expect).  Gaps between the blocks and the guards around a recv must come back unchanged
(sim_vhalves_api.run).
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import sim_vhalves_api as H
from test_kernel_resources import _kernels

AR, RS, AG, BC, RD, A2A = range(6)
AGV, RSV = H.ALLGATHERV, H.REDUCESCATTERV
DEFAULT_SLICE = 128 << 10  # MINI_NCCL_SLICE_SIZE's default
MODES = ("contig", "reversed", "gaps")


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_bound(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    for f, nargs in (("mncclAllGatherv", 8), ("mncclReduceScatterv", 9)):
        assert f in exported
        assert f in M.SIGNATURES and len(M.SIGNATURES[f][1]) == nargs
    assert callable(M.Comm.all_gather_v) and callable(M.Comm.reduce_scatter_v)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version


def _calls(L, M):
    fake, other = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)  # never dereferenced on these paths
    arr = (ctypes.c_size_t * 2)(4, 4)
    agv = lambda comm, c=arr, d=arr, dt=M.ncclFloat, op=None, s=fake, r=other: \
        L.mncclAllGatherv(s, 4, r, c, d, dt, comm, None)
    rsv = lambda comm, c=arr, d=arr, dt=M.ncclFloat, op=M.ncclSum, s=fake, r=other: \
        L.mncclReduceScatterv(s, c, d, r, 4, dt, op, comm, None)
    return fake, agv, rsv


def test_refusals_before_the_communicator_is_read(nccl_lib):
    """Checks 1 - 3 in their order, with a fake communicator that is never read."""
    import mini_nccl as M
    L = nccl_lib
    fake, agv, rsv = _calls(L, M)
    for call in (agv, rsv):
        # 1. a NULL comm or a NULL array: before the group, the datatype and the op
        assert call(None) == M.ncclInvalidArgument
        assert call(None, dt=M.ncclInt8, op=M.ncclAvg) == M.ncclInvalidArgument
        for k in ("c", "d"):
            assert call(fake, **{k: None}) == M.ncclInvalidArgument
            assert call(fake, dt=M.ncclInt8, **{k: None}) == M.ncclInvalidArgument
        # 3. an unsupported datatype: ncclInternalError before the communicator (a fake pointer) is
        #    read, and before the buffers are looked at (NULL buffers are the communicator's business)
        for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
            assert call(fake, dt=dt) == M.ncclInternalError
            assert call(fake, dt=dt, s=None, r=None) == M.ncclInternalError
    # 3. ncclAvg, and a value between the built-ins and the user handles' range that is neither
    assert rsv(fake, op=M.ncclAvg) == M.ncclInternalError
    assert rsv(fake, op=M.ncclAvg, s=None, r=None) == M.ncclInternalError
    assert rsv(fake, dt=M.ncclInt8, op=M.ncclAvg) == M.ncclInternalError
    assert rsv(fake, op=-1) == M.ncclInternalError
    # 2. an open group: ncclInvalidUsage after the NULL checks and BEFORE the datatype and the op; the
    #    group stays open and clean (its end succeeds and launches nothing: the fake is never read)
    assert L.ncclGroupStart() == 0
    try:
        for call in (agv, rsv):
            assert call(None) == M.ncclInvalidArgument
            assert call(fake, c=None) == M.ncclInvalidArgument
            assert call(fake) == M.ncclInvalidUsage
            assert call(fake, dt=M.ncclInt8) == M.ncclInvalidUsage
        assert rsv(fake, op=M.ncclAvg) == M.ncclInvalidUsage
    finally:
        assert L.ncclGroupEnd() == M.ncclSuccess
    assert L.ncclGroupEnd() == M.ncclInvalidUsage  # the group is closed
    assert agv(fake, dt=M.ncclInt8) == M.ncclInternalError  # and the checks are what they were


# ---------------------------------------------------------------- the host-side rules
def test_local_rules(sim_lib):
    a, o = 0x10000, 0x80000
    c, d, z = [4, 0, 7], [0, 4, 4], [0, 0, 0]
    top = (1 << 64) - 1
    for rank in (0, 2):
        assert H.check_local(rank, 4, a, c, d, o, c[rank]) == 0
    # the scalar count is the array's entry for `rank` -- checked first
    assert H.check_local(0, 4, a, c, d, o, 5) == 1
    assert H.check_local(1, 4, a, c, d, o, 1) == 1
    assert H.check_local(0, 4, None, c, d, None, 5) == 1
    # NULL buffers: fine where the counts are zero on that side, refused otherwise
    assert H.check_local(1, 4, a, c, d, None, 0) == 0      # an empty own block: no one-block buffer
    assert H.check_local(0, 4, None, z, z, None, 0) == 0   # every count zero: neither
    assert H.check_local(0, 4, None, z, d, o, 0) == 0
    assert H.check_local(0, 4, a, c, d, None, 4) == 2
    assert H.check_local(1, 4, None, c, d, None, 0) == 2   # the peers' blocks still need the array side
    # overflow: displ + count, the byte size, the address -- of the array side and of the one block
    assert H.check_local(0, 4, a, c, [top - 2, 0, 4], o, 4) == 3
    assert H.check_local(0, 4, a, [top // 4 + 1, 0, 0], z, o, top // 4 + 1) == 3
    assert H.check_local(0, 8, top - 15, [2, 0, 0], z, o, 2) == 3
    assert H.check_local(0, 8, a, [2, 0, 0], z, top - 15, 2) == 3
    assert H.check_local(0, 4, a, z, [top, top, top], None, 0) == 0  # empty blocks' displs are never used
    # overlapping blocks of the array side (the last element of block 0 is the first of block 2):
    # refused on both calls -- the rule has no side
    assert H.check_local(0, 4, a, c, [0, 4, 3], o, 4) == 4
    assert H.check_local(2, 4, a, c, [0, 0, 0], o, 7) == 4
    assert H.check_local(0, 4, a, c, [0, 1, 4], o, 4) == 0  # an empty block inside another overlaps nothing
    # the one-block buffer: the in-place form accepted, any other overlap refused
    assert H.check_local(0, 4, a, c, d, a, 4) == 0            # in place: block 0
    assert H.check_local(2, 4, a, c, d, a + 16, 7) == 0       # in place: block 2
    assert H.check_local(2, 4, a, c, d, a, 7) == 5            # block 2's buffer laid over block 0
    assert H.check_local(0, 4, a, c, d, a + 16, 4) == 5       # block 0's buffer laid over block 2
    assert H.check_local(0, 4, a, c, d, a + 4, 4) == 5        # partly over its own block
    assert H.check_local(2, 4, a, c, d, a + 43, 7) == 5       # by one byte
    assert H.check_local(2, 4, a, c, d, a + 44, 7) == 0       # merely adjacent
    assert H.check_local(0, 4, a + 100, c, [0, 4, 10], a + 116, 4) == 0  # in the gap between two blocks
    assert H.check_local(2, 2, a + 1, c, d, a + 23, 7) == 0   # odd addresses, adjacent
    # the order: count mismatch before NULL before overflow before block overlap before the one block
    assert H.check_local(0, 4, None, c, [top, 0, 0], None, 5) == 1
    assert H.check_local(0, 4, None, c, [top, 0, 0], o, 4) == 2
    assert H.check_local(0, 4, a, c, [top, 0, 3], a, 4) == 3
    assert H.check_local(0, 4, a, c, [0, 4, 3], a + 4, 4) == 4


def test_rows_must_be_equal(sim_lib):
    for n in (1, 2, 5, 16):
        c = np.random.default_rng(n).integers(0, 1000, n)
        C, D = np.tile(c, (n, 1)), np.tile(np.cumsum(c) - c, (n, 1))
        assert H.rows_differ(C, D) == 0
        for r, q in ((n - 1, 0), (n // 2, n - 1)):
            if r == 0:
                continue
            bad = C.copy()
            bad[r, q] += 1
            assert H.rows_differ(bad, D) == 1 + r * n + q
            bad = D.copy()
            bad[r, q] += 1
            assert H.rows_differ(C, bad) == 1 + r * n + q
    # an empty block's displacement counts too: the arrays must be identical
    assert H.rows_differ([[0, 1], [0, 1]], [[5, 0], [6, 0]]) == 1 + 2


def test_length_rule_against_numpy(sim_lib):
    L = H.load()
    blocks = [0, 1, 3, 15, 16, 17, 1023, 1024, 1025, 4096, 65644, (1 << 32) + 5]
    slices = [4, 16, 1024, 128 << 10, 256 << 20]
    for b in blocks:
        for sl in slices:
            full = b // sl
            ss = np.unique(np.clip(np.array([0, 1, 2, full - 1, full, full + 1, full + 2, 3 * full + 7], np.int64), 0, None))
            want = np.clip(b - ss * sl, 0, sl)  # the restatement: min(slice, what is left), never below 0
            got = [L.mnccl_vhalf_len(b, sl, int(s)) for s in ss]
            assert got == [int(x) for x in want], (b, sl)
    for b, sl in ((0, 16), (1, 16), (17, 16), (65644, 1024), (6, 1024)):
        lens = [L.mnccl_vhalf_len(b, sl, s) for s in range(b // sl + 3)]
        assert sum(lens) == b and lens == sorted(lens, reverse=True)  # full slices, one short one, zeros for good


def test_vector_path_rule(sim_lib):
    L = H.load()
    assert L.mnccl_vhalf_vec(1, 0, 16) == 1 and L.mnccl_vhalf_vec(1, 4, 20) == 1 and L.mnccl_vhalf_vec(1, 0, 0) == 1
    assert L.mnccl_vhalf_vec(0, 0, 16) == 0   # some rank's buffer is not dword-aligned
    assert L.mnccl_vhalf_vec(1, 2, 16) == 0   # an odd base
    assert L.mnccl_vhalf_vec(1, 4, 18) == 0   # an odd length


# ---------------------------------------------------------------- simulator
NS_SIM = [2, 3, 5, 8, 9]


def _shapes(n, sl_el):
    """The issue's cases at slice = sl_el elements: blocks that run out at different slices, a rank
    with an empty block, one rank holding everything, and (by the modes) gaps between the blocks."""
    ladder = [0, 1, sl_el - 1, sl_el, sl_el + 1, 3 * sl_el + 5]
    run_out = [ladder[(q * 5 + 2) % len(ladder)] for q in range(n)]
    empty = [sl_el + 3] * n
    empty[n // 2] = 0
    one_holds = [0] * n
    one_holds[n - 1] = 5 * sl_el + 1
    uniform = [2 * sl_el + 1] * n
    return [("run_out", run_out), ("empty", empty), ("one_holds", one_holds), ("uniform", uniform)]


def _one(n, coll, sched, shape, esz, slice_bytes, channels, seed, inplace, calls=1, min_slice=0, op="sum"):
    import oracle_api as O
    if coll == AGV:
        given = [shape.blocks(100 * seed + i, esz) for i in range(calls)]
    else:
        given = [O.random_inputs(n, shape.length, "f32", seed=3000 + 10 * seed + i) for i in range(calls)]
    outs = H.run(n, [(coll, sched, (shape, g), inplace, 0) for g in given], esz=esz, op=O.OPS[op], slice_bytes=slice_bytes,
                 channels=channels, seed=seed, min_slice=min_slice)
    what = f"n={n} coll={coll} sched={sched} counts={shape.counts} mode={shape.mode} slice={slice_bytes} C={channels} " \
           f"seed={seed} inplace={inplace}"
    for i, (g, out) in enumerate(zip(given, outs)):
        if coll == AGV:
            e = shape.gather_expect(g, esz)
            for q in range(n):
                assert np.array_equal(out[q], e), f"{what} call {i}: rank {q} differs (blocks or gaps)"
        else:
            for q, e in enumerate(shape.fold_expect(g, "f32", op)):
                assert np.array_equal(out[q].view(np.uint32), e.view(np.uint32)), f"{what} call {i}: rank {q} differs"


@pytest.mark.parametrize("sched", [H.RING, H.READ], ids=["ring", "read"])
@pytest.mark.parametrize("n", NS_SIM)
def test_sim_allgatherv(sim_lib, n, sched):
    seed = 0
    for slice_bytes in (16, 1024):
        for esz in (4, 2, 1):
            for name, counts in _shapes(n, slice_bytes // esz):
                seed += 1
                shape = H.Shape(counts, MODES[seed % 3])
                _one(n, AGV, sched, shape, esz, slice_bytes, (1, 4)[seed % 2], seed % 5, inplace=seed % 4 == 0,
                     calls=2 if seed % 3 == 0 else 1)
    # the adaptive slice of Comm::make_params (min_slice != 0), as the library picks it
    _one(n, AGV, sched, H.Shape([0, 16411] + [300] * (n - 2), "gaps"), 4, DEFAULT_SLICE, 4, 3, False, calls=2, min_slice=1024)


@pytest.mark.parametrize("sched", [H.RING, H.READ], ids=["ring", "read"])
@pytest.mark.parametrize("n", NS_SIM)
def test_sim_reducescatterv(sim_lib, oracle_lib, n, sched):
    seed = 0
    for slice_bytes in (16, 1024):
        for name, counts in _shapes(n, slice_bytes // 4):
            for op in ("sum", "max"):
                seed += 1
                shape = H.Shape(counts, MODES[seed % 3])
                _one(n, RSV, sched, shape, 4, slice_bytes, (1, 4)[seed % 2], seed % 5, inplace=seed % 4 == 0,
                     calls=2 if seed % 3 == 0 else 1, op=op)
    _one(n, RSV, sched, H.Shape([0, 16411] + [300] * (n - 2), "gaps"), 4, DEFAULT_SLICE, 4, 3, False, calls=2, min_slice=1024)


def test_sim_one_rank(sim_lib, oracle_lib):
    for sched in (H.RING, H.READ):
        for inplace in (False, True):
            _one(1, AGV, sched, H.Shape([37], "gaps"), 2, 16, 2, 1, inplace)
            _one(1, RSV, sched, H.Shape([37], "gaps"), 4, 16, 2, 1, inplace)
            _one(1, AGV, sched, H.Shape([0]), 4, 16, 2, 1, inplace)


def test_sim_uniform_counts_give_the_uniform_halves_exactly(sim_lib, oracle_lib):
    """Equal counts with contiguous displacements: the bits of the v forms are the uniform halves'."""
    import oracle_api as O
    import sim_alltoall_api as A
    for n in (2, 3, 8, 9):
        for count in (1, 300, 4099):
            for sched in (H.RING, H.READ):
                shape = H.Shape([count] * n)
                xs = O.random_inputs(n, n * count, "f32", seed=17 * n + count)
                (plain,) = A.run(n, [(RS, sched, xs, False, 0)], slice_bytes=1024, channels=4, seed=2)
                (var,) = H.run(n, [(RSV, sched, (shape, xs), False, 0)], slice_bytes=1024, channels=4, seed=2)
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, var)), (n, count, sched)
                ys = [x[:count] for x in xs]
                (plain,) = A.run(n, [(AG, sched, ys, False, 0)], slice_bytes=1024, channels=4, seed=2)
                (var,) = H.run(n, [(AGV, sched, (shape, [y.view(np.uint8) for y in ys]), False, 0)], slice_bytes=1024,
                               channels=4, seed=2)
                assert all(np.array_equal(a.view(np.uint8), b) for a, b in zip(plain, var)), (n, count, sched)


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("n,channels", [(2, 4), (3, 4), (5, 1), (8, 8), (9, 4)])
def test_sim_interleaved_with_the_other_collectives(sim_lib, oracle_lib, n, channels, seed):
    """18 calls on one communicator state: one of each of the six collectives with uniform counts,
    and between and after them the two v forms on both schedules, in and out of place.  Every call
    exact: the counters the schedules share stay in step."""
    import oracle_api as O
    import sim_alltoall_api as A
    from test_alltoall_cpu import _check as check_other
    g = np.random.default_rng(4000 * n + seed)
    sizes = (4099, 1, 1000, 256, 255, 700, 3)
    sl_el = 64  # 256-byte slices of 4-byte elements
    calls = []
    for i in range(18):
        coll = (AGV, RSV)[(i // 2) % 2] if i % 2 else (i // 2 + seed) % 6 if i < 12 else (RSV, AGV)[i % 4 // 2]
        sched = int(g.choice([H.RING, H.READ])) if i >= 4 else (H.RING, H.READ)[i // 2 % 2]
        root = int(g.integers(0, n))
        inplace = False
        if coll in (AGV, RSV):
            name, counts = _shapes(n, sl_el)[int(g.integers(0, 4))]
            counts = list(np.roll(counts, int(g.integers(0, n))))
            shape = H.Shape(counts, MODES[i % 3])
            inplace = bool(g.integers(0, 2))
            xs = (shape, shape.blocks(100 * seed + i, 4) if coll == AGV
                  else O.random_inputs(n, shape.length, "f32", seed=6000 * (seed + 1) + i))
        elif coll == A2A:
            xs = A.random_blocks(n, 4 * int(sizes[int(g.integers(0, len(sizes)))]), 100 * seed + i)
        else:
            c = int(sizes[int(g.integers(0, len(sizes)))])
            count = c if coll in (AG, BC, RD) else n * c + (3 if coll == AR else 0)
            xs = O.random_inputs(n, count, "f32", seed=5000 * (seed + 1) + i)
        calls.append((coll, sched, xs, inplace, root))
    assert {c[0] for c in calls} == set(range(6)) | {AGV, RSV} and {c[1] for c in calls} == {H.RING, H.READ}
    outs = H.run(n, calls, slice_bytes=256, channels=channels, slots=2, seed=seed)
    for i, ((coll, sched, xs, inplace, root), out) in enumerate(zip(calls, outs)):
        what = f"call {i} (coll {coll}, schedule {sched}, root {root}, in place {inplace})"
        if coll == AGV:
            e = xs[0].gather_expect(xs[1], 4)
            for q in range(n):
                assert np.array_equal(out[q], e), f"{what}: rank {q} differs"
        elif coll == RSV:
            for q, e in enumerate(xs[0].fold_expect(xs[1])):
                assert np.array_equal(out[q].view(np.uint32), e.view(np.uint32)), f"{what}: rank {q} differs"
        else:
            check_other(coll, xs, root, out, what)


def test_existing_entry_points_keep_their_ranges(sim_lib):
    """mnccl_sim_all_collectives refuses collectives 9 and 10 as it refused everything past 8;
    mnccl_sim_vhalves takes them and refuses the variable all-to-all, which it has no matrices for."""
    import sim_gather_scatter_api as G
    shape = H.Shape([1, 2])
    for coll in (AGV, RSV):
        with pytest.raises(ValueError):
            G.run(2, [(coll, H.RING, [np.zeros(4, np.float32)] * 2, False, 0)])
    with pytest.raises(ValueError):
        H.run(2, [(6, H.RING, [np.zeros(4, np.float32)] * 2, False, 0)])
    blocks = shape.blocks(1, 4)
    (out,) = H.run(2, [(AGV, H.RING, (shape, blocks), False, 0)])
    assert all(np.array_equal(o, shape.gather_expect(blocks, 4)) for o in out)


# ---------------------------------------------------------------- kernel resources
def test_new_kernels_fit_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    all_ks = _kernels(tmp_path)
    ks = {k: v for k, v in all_ks.items() if "vhalf" in k}
    # vhalf_fold: 5 datatypes x 4 ops x (vector, element); scaled_vhalf: 5 x 2; vhalf_fp8: 2 x 5 ops x 2;
    # vhalf_push: element sizes 2 / 4 / 8 x 2; vhalf_byte: 2
    assert len(ks) == 40 + 10 + 20 + 6 + 2, sorted(ks)
    for k, v in ks.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the existing counts are what they were, and the new names stay out of them
    old = re.compile(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push")
    assert not [k for k in ks if old.search(k)]
    assert len([k for k in all_ks if old.search(k)]) == 5 * 40 + 3 * 6
