"""The case table of the batch-boundary GPU tests (tests/boundary_cases.py) against the library's own
slicing: for every case, the slices each rank's call runs -- (nvec, tail bytes) per pipeline -- are
computed with the simulator library's read_slice / effective_slice / call_pipelines, and every class
the GPU test is there for must be among them.  A change to the slicing that moves the cases off the
batch boundaries fails here; without this the GPU test could pass vacuously.
"""
import pytest

import boundary_cases as B
import sim_api as S

DEFAULT_SLICE = 128 << 10  # config.h slice_size
MIN_SLICE = 1024           # schedule.h kMinSlice
READ_DEPTH = 16            # schedule.h kReadDepth

# Vectors per batch of the read schedule's fold, 64 * V (kernels.hip read_fold: V = 12 - 4h at n = 2,
# 8 - 2h at 3, 4 - h up to 5, 3 - h up to 8, h = 1 for the 2-byte types); past 8 ranks full batches of
# 64 * kReadFoldU = 1024, then read_fold_wide's steps of 64 * kWideV = 128.
FOLD_S = {(2, 4): 768, (2, 2): 512, (3, 4): 512, (3, 2): 384, (5, 4): 256, (5, 2): 192, (8, 4): 192, (8, 2): 128}
# gather_push_vec / relay_vec / exchange_push_vec: 64 * kGatherV = 64 * kExchangeV = 512
PUSH_S = 512
# move_vec: full batches of 64 * kU = 512, then single vectors
MOVE_CLASSES = {511, 512, 513, 1024, 1025}
LOOP = {"rs": "fold", "ar": "fold", "rd": "fold", "ag": "push", "bc": "push", "a2a": "push"}


def slice_len(chunk, sl, s):  # schedule.h slice_len
    return 0 if s * sl >= chunk else min(sl, chunk - s * sl)


def rooted_len(total, chunk_off, chunk, sl, s):  # schedule.h rooted_len
    off = chunk_off + s * sl
    return 0 if off >= total else min(slice_len(chunk, sl, s), total - off)


def _per_rank(v, r):
    return v[r % len(v)] if isinstance(v, (list, tuple)) else v


def plan(case, n, env, pipes=None):
    """What Comm::launch and the kernels make of one case: {"vec", "A", "iters", "ranks": per rank the
    list of (pipeline, nvec, tail bytes) of its non-empty messages}."""
    esz = B.ESZ[case["dtype"]]
    coll, count, ring = case["coll"], case["count"], case["algo"] == B.RING
    C = pipes or int(env.get("MINI_NCCL_CHANNELS", 0))
    cfg_slice = int(env.get("MINI_NCCL_SLICE_SIZE", DEFAULT_SLICE))
    rooted = coll in ("bc", "rd")
    total = count * esz
    chunk = -(-count // n) * esz if rooted else total
    if ring and coll == "bc":
        chunk = total  # the ring's broadcast moves the whole buffer as one chunk
    sl = S.effective_slice(chunk, C, cfg_slice, MIN_SLICE, 1) if ring else S.read_slice(chunk, C, cfg_slice, MIN_SLICE, READ_DEPTH)
    nslices = -(-chunk // sl)
    A = S.call_pipelines(nslices, C, 1)
    iters = -(-nslices // A)
    offs = [case.get("offset", 0), case.get("recv_offset", case.get("offset", 0))]
    vec = chunk % 4 == 0 and all(_per_rank(o, r) % 4 == 0 for o in offs for r in range(n))
    ranks = []
    for r in range(n):
        # the read schedule: rank r works on chunk r; the ring's Reduce passes every chunk through every rank
        chunks = [r] if not ring else range(n) if coll == "rd" else [0]
        msgs = []
        for s in range(A * iters):  # slice s: pipeline s mod A, iteration s / A
            for c in chunks:
                ln = rooted_len(total, c * chunk, chunk, sl, s) if rooted and not (ring and coll == "bc") else slice_len(chunk, sl, s)
                if ln:
                    msgs.append((s % A, ln // 16, ln % 16))
        ranks.append(msgs)
    return {"vec": vec, "A": A, "iters": iters, "ranks": ranks}


def hits(group, coll, esz_class, ring=False):
    """(nvec, tail) of the vector path's slices, and the byte lengths of the element path's, over
    the group's cases of one collective and element-size class (2, or 4 for the 4- and 8-byte types)."""
    vec, elem = set(), set()
    for case in group["cases"]:
        esz = B.ESZ[case["dtype"]]
        if case["coll"] != coll or (2 if esz == 2 else 4) != esz_class or (case["algo"] == B.RING) != ring:
            continue
        p = plan(case, group["n"], group["env"], group.get("pipes"))
        for msgs in p["ranks"]:
            for _, nvec, tail in msgs:
                (vec if p["vec"] else elem).add((nvec, tail) if p["vec"] else nvec * 16 + tail)
    return vec, elem


@pytest.mark.parametrize("name", [k for k in B.GROUPS if not k.startswith(("ring-small", "align"))])
def test_every_case_ends_on_the_class_it_names(sim_lib, name):
    """Case by case: rank 0's last slice is the case's `last` (and every rank's, where the count is
    n * q or the collective is not rooted) -- one vector more or less in any single case fails here."""
    g = B.GROUPS[name]
    n = g["n"]
    pipes = B.RING_DEFAULT_PIPES if name.startswith("ring-default") else None
    for c in g["cases"]:
        if "clamp" in c:
            continue  # test_rooted_chunk_shapes
        p = plan(c, n, g["env"], pipes)
        assert p["ranks"][0][-1][1:] == tuple(c["last"]), (c, p["ranks"][0][-1])
        if not (c["coll"] in ("bc", "rd") and c["count"] % n):
            assert all(m[-1][1:] == tuple(c["last"]) for m in p["ranks"]), c
        if c["last"][0] * 16 + c["last"][1] <= 16384 and g["env"] == B.ONE:
            assert all(len(m) == 1 for m in p["ranks"]), c  # the one slice of the chunk


def _assert_classes(name, coll, esz_class, want, tailed, vec, elem):
    """want: the classes' nvec; tailed: the ones of which at least one must carry a sub-vector tail"""
    got = {v for v, _ in vec}
    assert want <= got, f"{name} {coll} esz {esz_class}: classes {sorted(want - got)} not hit (hit: {sorted(got)})"
    assert any(v in tailed and t for v, t in vec), f"{name} {coll} esz {esz_class}: no sub-vector tail at {sorted(tailed)}"
    if esz_class == 2:
        assert any(b % 4 == 2 for b in elem), f"{name} {coll}: no 2-byte case with nbytes % 4 == 2"


@pytest.mark.parametrize("n", B.READ_NS)
def test_read_groups_hit_every_class(sim_lib, n):
    name = f"read-n{n}"
    g = B.GROUPS[name]
    assert g["env"] == B.ONE and g["n"] == n
    for esz_class in (4, 2):
        if n > 8:
            fold, fold_tailed = {1023, 1024, 1025, 1024 + 127, 1024 + 128, 1024 + 129}, {1025}
        else:
            s = FOLD_S[(n, esz_class)]
            fold, fold_tailed = {s - 1, s, s + 1, 2 * s, 2 * s + 1, 3 * s + 1}, {s + 1, 2 * s + 1}
        push = {PUSH_S - 1, PUSH_S, PUSH_S + 1, 2 * PUSH_S, 2 * PUSH_S + 1, 3 * PUSH_S + 1}
        for coll in ("rs", "ar", "rd"):
            _assert_classes(name, coll, esz_class, fold, fold_tailed, *hits(g, coll, esz_class))
        for coll in ("ag", "bc", "a2a"):
            want = push | {3 * PUSH_S} if coll == "a2a" else push
            _assert_classes(name, coll, esz_class, want, {PUSH_S + 1, 2 * PUSH_S + 1}, *hits(g, coll, esz_class))
    # the f64 max and f16 prod cases: S + 1 vectors and a tail, on the vector path
    for dt, op in (("f64", "max"), ("f16", "prod")):
        s1 = 1025 if n > 8 else FOLD_S[(n, 2 if B.ESZ[dt] == 2 else 4)] + 1
        for coll in ("rs", "ar", "rd"):
            cs = [c for c in g["cases"] if c["coll"] == coll and c["dtype"] == dt and c["op"] == op]
            assert cs, (coll, dt)
            for c in cs:
                p = plan(c, n, g["env"])
                _, nvec, tail = p["ranks"][0][-1]
                assert p["vec"] and nvec == s1 and tail, (c, nvec, tail)


@pytest.mark.parametrize("n", B.READ_NS)
def test_rooted_chunk_shapes(sim_lib, n):
    """count = n * q: every rank's chunk runs the same slices; the clamp cases: the last rank's last
    slice is S + 1 vectors and a tail, every other rank's is longer."""
    g = B.GROUPS[f"read-n{n}"]
    clamps = {"rd": set(), "bc": set()}
    for c in g["cases"]:
        if c["coll"] not in ("rd", "bc"):
            continue
        p = plan(c, n, g["env"])
        if "clamp" not in c:
            assert c["count"] % n == 0 and all(m == p["ranks"][0] for m in p["ranks"]), c
            continue
        nvec, tail = c["clamp"]
        s1 = PUSH_S + 1 if c["coll"] == "bc" else 1025 if n > 8 else FOLD_S[(n, 2 if B.ESZ[c["dtype"]] == 2 else 4)] + 1
        assert p["vec"] and nvec == s1 and tail
        assert p["ranks"][n - 1][-1][1:] == (nvec, tail), (c, p["ranks"][n - 1][-1])
        for r in range(n - 1):
            w, nv, t = p["ranks"][r][-1]
            assert nv * 16 + t > nvec * 16 + tail, (c, r)
        clamps[c["coll"]].add((B.ESZ[c["dtype"]], c["root"]))
    for coll in ("rd", "bc"):
        assert clamps[coll] == {(e, root) for e in (4, 2) for root in (0, n - 1)}, (coll, clamps[coll])


@pytest.mark.parametrize("n", B.ROT_NS)
def test_rotation_groups_run_ragged_batches_on_several_pipelines(sim_lib, n):
    """Slices of 513 vectors on 4 pipelines: the pushes' first destination, w mod (n - 1), takes more
    than one value among the pipelines that run a ragged batch sequence, and one pipeline runs three
    iterations (the all-to-all's parity carries over destinations and iterations)."""
    g = B.GROUPS[f"rot-n{n}"]
    assert g["env"] == B.ROT
    for coll in ("rs", "ar", "rd", "ag", "bc", "a2a"):
        for esz_class in (4, 2):
            vec, _ = hits(g, coll, esz_class)
            assert {513, 512, 511} <= {v for v, _ in vec}, (coll, esz_class, sorted(vec))
            assert (511, 4) in vec, (coll, esz_class)
    seen_iters = set()
    for c in g["cases"]:
        p = plan(c, n, g["env"])
        assert p["vec"] and p["A"] == 4, (c, p["A"])
        seen_iters.add(p["iters"])
        for msgs in p["ranks"]:
            ragged = {w % (n - 1) for w, nvec, _ in msgs if nvec % PUSH_S}
            assert len(ragged) > 1, (c, ragged)
    assert seen_iters == {2, 3}


@pytest.mark.parametrize("n", B.RING_NS)
def test_ring_small_groups_run_many_iterations(sim_lib, n):
    g = B.GROUPS[f"ring-small-n{n}"]
    assert g["env"] == B.SMALL
    for coll in ("rs", "ag", "bc", "rd", "a2a"):
        its = [plan(c, n, g["env"])["iters"] for c in g["cases"] if c["coll"] == coll]
        assert all(c["algo"] == B.RING for c in g["cases"])
        assert min(its) == 1 and max(its) >= 16, (coll, its)  # 2 slots: the FIFO wraps 8 times and more


def test_ring_default_group_hits_move_vec_classes(sim_lib):
    """At the default geometry the communicator has 256 pipelines at n = 5 and a call may launch all
    of them, whether the ranks share one 256-CU GPU or not; the chunks then give move_vec 511 / 512 /
    513 / 1024 / 1025 vectors, for every collective."""
    n = B.RING_DEFAULT_N
    g = dict(B.GROUPS[f"ring-default-n{n}"], pipes=B.RING_DEFAULT_PIPES)
    assert g["env"] == {}
    geo = S.pipeline_geometry(n)
    assert geo["workgroups"] * geo["waves"] == B.RING_DEFAULT_PIPES and geo["slot_bytes"] == DEFAULT_SLICE
    assert S.resident_pipes(B.RING_DEFAULT_PIPES, 1, 256, n) == B.RING_DEFAULT_PIPES
    assert S.resident_pipes(B.RING_DEFAULT_PIPES, 1, 256, 1) == B.RING_DEFAULT_PIPES
    for coll in ("rs", "ag", "bc", "rd", "a2a"):
        vec, _ = hits(g, coll, 4, ring=True)
        assert MOVE_CLASSES <= {v for v, _ in vec}, (coll, sorted(vec))
        assert (513, 4) in vec, coll
        vec2, _ = hits(g, coll, 2, ring=True)
        assert (513, 4) in vec2, coll


@pytest.mark.parametrize("n", B.ALIGN_NS)
def test_alignment_groups(n):
    """Every collective on both schedules with a different dword-aligned 16-byte phase per rank and
    buffer, and with rank 1 alone 2-byte-misaligned under a 2-byte type."""
    g = B.GROUPS[f"align-n{n}"]
    for algo in (B.READ, B.RING):
        for coll in ("rs", "ag", "ar", "bc", "rd", "a2a"):
            cs = [c for c in g["cases"] if c["algo"] == algo and c["coll"] == coll]
            phase = [c for c in cs if "recv_offset" in c]
            odd = [c for c in cs if "recv_offset" not in c]
            assert {c["dtype"] for c in phase} == {"f32", "bf16"} and odd, (algo, coll)
            for c in phase:
                so, ro = c["offset"], c["recv_offset"]
                assert so == [4 * (r % 4) for r in range(n)] and ro == [4 * ((r + 1) % 4) for r in range(n)]
                assert len({o % 16 for o in so}) > 1 and all(s != r for s, r in zip(so, ro))
                assert B.ESZ[c["dtype"]] * -(-c["count"] // (n if coll in ("bc", "rd") else 1)) % 4 == 0
            for c in odd:
                assert B.ESZ[c["dtype"]] == 2 and c["offset"] == [2 if r == 1 else 0 for r in range(n)]


def test_every_case_is_seeded_apart():
    for name, g in B.GROUPS.items():
        seeds = [c["seed"] for c in g["cases"]]
        assert len(set(seeds)) == len(seeds), name
