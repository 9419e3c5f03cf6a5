"""The batch-boundary cases of tests/test_boundaries_gpu.py, as plain data (no HIP, no library).

The read schedule's double-buffered loops (kernels.hip read_fold_all, gather_push_vec, relay_vec,
exchange_push_vec) move a slice of nvec 16-byte vectors in batches of S = 64 * V vectors, load the
next batch unconditionally and leave after either register set; read_fold past 8 ranks runs full
batches of 1024 and then read_fold_wide in steps of 128; the ring's move_vec full batches of 512
and then single vectors.  The cases here put a slice's nvec on the boundaries of those batches:

    S - 1, S, S + 1 (with a sub-vector tail), 2S, 2S + 1, 3S + 1            the double-buffered loops
    1023, 1024, 1025 (tail), 1024 + 127, 1024 + 128, 1024 + 129             the fold past 8 ranks
    511, 512, 513, 1024, 1025                                               move_vec

tests/test_boundary_cases.py computes, with the library's own read_slice / effective_slice /
call_pipelines, the slices every rank's call runs for every case below and asserts that each class
is hit for each (loop, n, element size): a change to the slicing that moves these cases off the
boundaries fails there, not silently here.

A GROUP is one communicator: n ranks, an environment and the cases run on it in order.  A case is
what alltoall_workers.a2a_rank takes: coll ("rs" / "ag" / "ar": count per rank; "bc" / "rd": count
in the whole buffer; "a2a": count per block), dtype, op, count, inplace, algo, root, null, seed and
the per-rank offset / recv_offset lists.  For the CPU test alone: last, the (nvec, tail bytes) the
case is there for -- rank 0's last slice -- and clamp, the same of the last rank's clamped chunk.
"""
RING, READ = 0, 2
ESZ = {"f32": 4, "f64": 8, "i32": 4, "f16": 2, "bf16": 2}
READ_NS = (2, 3, 5, 8, 9)   # one per G instantiation of the fold and the pushes, and the loop form past 8
ROT_NS = (3, 5, 9)
RING_NS = (2, 5, 8, 9)
ALIGN_NS = (3, 5)
RING_DEFAULT_N = 5

# one pipeline, the default 128 KiB slice: a chunk of at most 16 KiB is ONE slice of exactly the
# chunk's bytes; a longer one (chunk_bytes below) 15 equal slices and a last one of the wanted length
ONE = {"MINI_NCCL_CHANNELS": "1"}
# four pipelines, slices of 513 vectors: the pushes' rotation w mod (n - 1) takes several values
# while every batch sequence is ragged
ROT = {"MINI_NCCL_CHANNELS": "4", "MINI_NCCL_SLICE_SIZE": "8208"}
ROT_SLICE = 8208
# the suite's small geometry: 1 KiB slices, 4 pipelines (2 slots: the default)
SMALL = {"MINI_NCCL_SLICE_SIZE": "1024", "MINI_NCCL_CHANNELS": "4"}

PUSH_BATCH = 512  # gather_push_vec / relay_vec / exchange_push_vec: 64 lanes x 8 vectors


def fold_batch(n, esz):
    """Vectors per batch of the fold at n ranks (this table's own copy: the CPU test has another)."""
    two = esz == 2
    if n == 2:
        return 512 if two else 768
    if n == 3:
        return 384 if two else 512
    if n <= 5:
        return 192 if two else 256
    if n <= 8:
        return 128 if two else 192
    return 1024


def classes(S, tail):
    """(nvec, tail bytes) of the double-buffered loops' classes; S + 1 carries the tail."""
    return [(S - 1, 0), (S, 0), (S + 1, tail), (2 * S, 0), (2 * S + 1, 0), (3 * S + 1, 0)]


def wide_classes(tail):
    """The fold past 8 ranks: full batches of 1024, then read_fold_wide's steps of 128."""
    return [(1023, 0), (1024, 0), (1025, tail), (1024 + 127, 0), (1024 + 128, 0), (1024 + 129, 0)]


def fold_classes(n, esz, tail):
    return wide_classes(tail) if n > 8 else classes(fold_batch(n, esz), tail)


def chunk_bytes(nvec, tail=0):
    """A chunk whose only or last slice under ONE is nvec vectors and `tail` bytes long."""
    want = nvec * 16 + tail
    if want <= 16384:
        return want
    full = (want + 1023) // 1024 * 1024  # read_slice: ceil(chunk / 16) in whole KiB
    return 15 * full + want


def _case(coll, dtype, count, algo=READ, op="sum", inplace=False, root=0, **kw):
    return dict(coll=coll, dtype=dtype, op=op, count=count, inplace=inplace, algo=algo, root=root, **kw)


def _seeded(cases, base):
    return [dict(c, seed=base + i) for i, c in enumerate(cases)]


def read_cases(n):
    """Every class of every loop at n ranks, one pipeline (ONE)."""
    out = []
    roots = (0, n - 1)
    # the folds: reduce-scatter, all-reduce, reduce
    for dt, tail in (("f32", 4), ("bf16", 12)):
        esz = ESZ[dt]
        cls = fold_classes(n, esz, tail)
        if esz == 2:
            cls = cls + [(cls[2][0], 2)]  # chunk bytes = 2 mod 4: the element path at the same length
        for i, (nvec, t) in enumerate(cls):
            c = chunk_bytes(nvec, t) // esz
            for inplace in (False, True):
                out.append(_case("rs", dt, c, inplace=inplace, last=(nvec, t)))
                out.append(_case("ar", dt, c, inplace=inplace, last=(nvec, t)))
            for j, root in enumerate(roots):  # count = n * q: every rank's chunk is the class
                out.append(_case("rd", dt, n * c, inplace=(i + j) % 2 == 1, root=root, null=(i + j) % 2 == 0, last=(nvec, t)))
    for dt, op, tail in (("f64", "max", 8), ("f16", "prod", 4)):
        esz = ESZ[dt]
        nvec, t = fold_classes(n, esz, tail)[2]
        c = chunk_bytes(nvec, t) // esz
        out += [_case("rs", dt, c, op=op, last=(nvec, t)), _case("ar", dt, c, op=op, inplace=True, last=(nvec, t)),
                _case("rd", dt, n * c, op=op, root=n - 1, null=True, last=(nvec, t))]
    # the pushes: all-gather, broadcast, all-to-all
    for dt, tail in (("f32", 4), ("bf16", 12)):
        esz = ESZ[dt]
        cls = classes(PUSH_BATCH, tail)
        if esz == 2:
            cls = cls + [(cls[2][0], 2)]
        for i, (nvec, t) in enumerate(cls):
            c = chunk_bytes(nvec, t) // esz
            for inplace in (False, True):
                out.append(_case("ag", dt, c, inplace=inplace, last=(nvec, t)))
            for j, root in enumerate(roots):
                out.append(_case("bc", dt, n * c, inplace=(i + j) % 2 == 1, root=root, null=(i + j) % 2 == 0, last=(nvec, t)))
            out.append(_case("a2a", dt, c, last=(nvec, t)))
        # three whole batches per destination
        out.append(_case("a2a", dt, chunk_bytes(3 * PUSH_BATCH) // esz, last=(3 * PUSH_BATCH, 0)))
    # the rooted collectives' clamp: count = n * q - 1, so the last rank's chunk is one element
    # short -- S + 1 vectors and a tail -- while the others' are longer
    for dt, tail in (("f32", 4), ("bf16", 6)):
        esz = ESZ[dt]
        for coll, (nvec, _) in (("rd", fold_classes(n, esz, 0)[2]), ("bc", classes(PUSH_BATCH, 0)[2])):
            q = chunk_bytes(nvec, tail + esz) // esz
            for j, root in enumerate(roots):
                out.append(_case(coll, dt, n * q - 1, inplace=j == 1, root=root, null=j == 0, clamp=(nvec, tail)))
    return _seeded(out, 100)


def rot_cases(n):
    """Four pipelines, slices of 513 vectors (ROT): 5 slices, the last 511 vectors and 4 bytes, and
    9 slices, the last exactly one batch -- pipeline 0 runs three iterations."""
    out = []
    for dt in ("f32", "bf16"):
        esz = ESZ[dt]
        for cb, last in ((4 * ROT_SLICE + 511 * 16 + 4, (511, 4)), (8 * ROT_SLICE + 512 * 16, (512, 0))):
            c = cb // esz
            new = [_case("rs", dt, c), _case("ar", dt, c, inplace=True), _case("ag", dt, c), _case("ag", dt, c, inplace=True),
                   _case("bc", dt, n * c, root=0, null=True), _case("bc", dt, n * c, root=n - 1, inplace=True),
                   _case("bc", dt, n * c - 1, root=1), _case("rd", dt, n * c, root=n - 1, null=True),
                   _case("rd", dt, n * c - 1, root=0, inplace=True), _case("a2a", dt, c)]
            out += [dict(x, last=last) for x in new]
    return _seeded(out, 300)


def ring_small_cases(n):
    """The five newer collectives on the ring with 1 KiB slices on 4 pipelines over 2 slots: 300 and
    16411 elements per chunk (17 iterations per pipeline; a Reduce's last chunk one element short, a
    Broadcast's buffer the ring's one chunk)."""
    out = []
    for dt in ("f32", "bf16"):
        for c in (300, 16411):
            out += [_case("rs", dt, c, RING, inplace=c == 300), _case("ag", dt, c, RING, inplace=c != 300),
                    _case("bc", dt, c, RING, root=0, null=True), _case("bc", dt, c, RING, root=n - 1, inplace=True),
                    _case("rd", dt, n * c - 1, RING, root=0, inplace=True), _case("rd", dt, n * c - 1, RING, root=n - 1, null=True),
                    _case("a2a", dt, c, RING)]
    return _seeded(out, 500)


# the ring at the default geometry and n = RING_DEFAULT_N: 256 pipelines (one per CU; also what
# resident_pipes leaves with the 5 ranks on one GPU), so effective_slice is ceil(chunk / 256) in whole
# KiB -- 255 slices of that and a last one of (last vectors, tail bytes)
RING_DEFAULT_PIPES = 256
RING_DEFAULT_CHUNKS = [(8192, 511, 0), (9216, 513, 4), (17408, 1025, 0), (17408, 1024, 0)]


def ring_default_cases(n=RING_DEFAULT_N):
    out = []
    for i, (sl, last, tail) in enumerate(RING_DEFAULT_CHUNKS):
        cb = (RING_DEFAULT_PIPES - 1) * sl + last * 16 + tail
        for dt in ("f32", "bf16") if i == 1 else ("f32",):
            c = cb // ESZ[dt]
            new = [_case("rs", dt, c, RING, inplace=i % 2 == 0), _case("ag", dt, c, RING, inplace=i % 2 == 1),
                   _case("bc", dt, c, RING, root=0, null=True), _case("bc", dt, c, RING, root=n - 1, inplace=True),
                   _case("rd", dt, n * c, RING, root=0, inplace=True), _case("rd", dt, n * c, RING, root=n - 1, null=True),
                   _case("a2a", dt, c, RING)]
            out += [dict(x, last=(last, tail)) for x in new]
    return _seeded(out, 700)


def align_cases(n):
    """A base per rank and per buffer.  phase: rank r's send 4 * (r mod 4) bytes and its recv
    4 * ((r + 1) mod 4) bytes into its allocation -- dword-aligned, a different 16-byte phase on every
    rank and buffer: the vector path.  odd: rank 1 alone on a 2-byte-misaligned base with a 2-byte
    type: every rank takes the element path.  Both schedules; in place the one offset serves both."""
    phase = dict(offset=[4 * (r % 4) for r in range(n)], recv_offset=[4 * ((r + 1) % 4) for r in range(n)])
    odd = dict(offset=[2 if r == 1 else 0 for r in range(n)])
    out = []
    for algo in (READ, RING):
        for dt, c, kw in (("f32", 4099, phase), ("bf16", 4100, phase), ("bf16", 4100, odd)):
            for inplace in (False, True):
                out += [_case("rs", dt, c, algo, inplace=inplace, **kw), _case("ag", dt, c, algo, inplace=inplace, **kw),
                        _case("ar", dt, c, algo, inplace=inplace, **kw)]
                for root in (0, 1):  # rank 1: the misaligned rank as the root
                    out += [_case("bc", dt, n * c - 1, algo, inplace=inplace, root=root, null=not inplace, **kw),
                            _case("rd", dt, n * c - 1, algo, inplace=inplace, root=root, null=inplace, **kw)]
            out.append(_case("a2a", dt, c, algo, **kw))
    return _seeded(out, 900)


GROUPS = {}
for _n in READ_NS:
    GROUPS[f"read-n{_n}"] = dict(n=_n, env=ONE, cases=read_cases(_n))
for _n in ROT_NS:
    GROUPS[f"rot-n{_n}"] = dict(n=_n, env=ROT, cases=rot_cases(_n))
for _n in RING_NS:
    GROUPS[f"ring-small-n{_n}"] = dict(n=_n, env=SMALL, cases=ring_small_cases(_n))
GROUPS[f"ring-default-n{RING_DEFAULT_N}"] = dict(n=RING_DEFAULT_N, env={}, cases=ring_default_cases())
for _n in ALIGN_NS:
    GROUPS[f"align-n{_n}"] = dict(n=_n, env={}, cases=align_cases(_n))
