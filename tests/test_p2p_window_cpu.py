"""ncclSend / ncclRecv into registered windows without a GPU (-m "not gpu"): the window kernel's protocol
and data in the simulator (csrc/sim.cpp mnccl_sim_p2p_win: a DEST record per message on the real word
layout, direct pushes and scratch slices on one counter state), the pure functions csrc/p2p.h adds
(slot assignment, the direct / scratch decision, the DEST record and its check), the mailbox layout,
and the new kernel's resource budget read from the library.

Every recv lies in one of two arenas per rank -- the registered window, or a plain buffer outside it
-- with 64 guard bytes of fill on both sides of every range; after a run BOTH arenas equal their
expected image byte for byte, so nothing but the recv ranges was written.  The final counters equal
those of the all-scratch run of the same program on csrc/sim.cpp mnccl_sim_p2p (the kernel without
windows): a direct message consumes exactly the sequence numbers its scratch form would.
"""
import numpy as np
import pytest

import sim_p2p_api as P
import sim_p2p_win_api as PW
from test_kernel_resources import _kernels

FILL, GUARD = 0xA5, 64
# the geometry of tests/test_p2p_cpu.py: 2 slots, 2 pipelines, 1 KiB slots; every message may use both
SLOTS, C, SLOT, A = 2, 2, 1024, 2
SIZES = (700, SLOTS * A * SLOT, 3 * SLOTS * A * SLOT + 20)
LARGEST = SIZES[-1]
SEEDS = [0, 1, 5]
MODES = {"direct": lambda k: True, "scratch": lambda k: False, "alternating": lambda k: k % 2 == 0}


def _bytes(seed, *key, size):
    return np.frombuffer(np.random.default_rng([seed, *key]).bytes(size), np.uint8).copy()


class Arena:
    """One buffer of fill bytes; take() hands out ranges with GUARD fill bytes on both sides and
    records what each must hold afterwards."""

    def __init__(self, size):
        self.buf = np.full(size, FILL, np.uint8)
        self.want = self.buf.copy()
        self.at = GUARD

    def take(self, payload):
        off, self.at = self.at, self.at + payload.size + GUARD
        assert self.at <= self.buf.size
        self.want[off:off + payload.size] = payload
        return self.buf[off:off + payload.size]

    def ok(self):
        return np.array_equal(self.buf, self.want)


class Ranks:
    """n ranks, each with a registered window (window 0) and a plain arena."""

    def __init__(self, n, size=1 << 17):
        self.n = n
        self.win = [Arena(size) for _ in range(n)]
        self.plain = [Arena(size) for _ in range(n)]

    def recv(self, r, peer, payload, direct):
        return ("recv", peer, (self.win if direct else self.plain)[r].take(payload), 0 if direct else None)

    @staticmethod
    def send(peer, payload):
        return ("send", peer, payload, None)

    def windows(self):
        return [[a.buf for a in self.win]]

    def ok(self):
        return all(a.ok() for a in self.win + self.plain)


def _run(n, phases, R, seed):
    return PW.run(n, phases, R.windows(), channels=C, slots=SLOTS, slot_bytes=SLOT, pipes=A, seed=seed)


def _scratch_counters(n, phases, seed):
    """The same program on the kernel without windows (fresh recv buffers: only the counters matter)."""
    old = []
    for ph in phases:
        if not isinstance(ph, dict):
            old.append(ph)
            continue
        old.append({r: [[(k, p, b if k == "send" else np.empty_like(b)) for k, p, b, _ in launch] for launch in ls]
                    for r, ls in ph.items()})
    _, tx, rx = P.run(n, old, channels=C, slots=SLOTS, slot_bytes=SLOT, pipes=A, seed=seed)
    return tx, rx


def _three_to_one_peer(R, seed, tag, size, mode):
    """Every rank sends three messages (size, 700 B, the largest) to r + 1 in one group and receives
    three from r - 1; message k is direct where mode(k)."""
    n, sizes = R.n, (size, 700, LARGEST)
    msgs = [[_bytes(seed, tag, r, k, size=s) for k, s in enumerate(sizes)] for r in range(n)]
    return {r: [[R.send((r + 1) % n, m) for m in msgs[r]] +
                [R.recv(r, (r - 1) % n, m, MODES[mode](k)) for k, m in enumerate(msgs[(r - 1) % n])]]
            for r in range(n)}


# ---------------------------------------------------------------- simulator
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [2, 3, 5])
def test_sim_groups_between_ring_collectives(sim_lib, n, mode, size, seed):
    """A ring all-reduce, a group of three messages to one peer (all direct / all scratch in the new
    kernel / direct, scratch, direct), the all-reduce again, the group again: the bytes, the guards,
    the all-reduces' sums, and the counters of the all-scratch run."""
    R = Ranks(n)
    g = np.random.default_rng(seed)
    ins = [g.integers(-1000, 1000, n * 1100).astype(np.float32) for _ in range(n)]
    phases = [("ar", P.RING, ins), _three_to_one_peer(R, seed, 1, size, mode), ("ar", P.RING, ins),
              _three_to_one_peer(R, seed, 2, size, mode)]
    outs, tx, rx, direct = _run(n, phases, R, seed)
    assert R.ok()
    for i in (0, 2):
        for r in range(n):
            assert np.array_equal(outs[i][r], sum(ins)), (i, r)
    tx0, rx0 = _scratch_counters(n, phases, seed)
    assert np.array_equal(tx, tx0) and np.array_equal(rx, rx0)
    per_group = sum(1 for k in range(3) if MODES[mode](k))
    assert direct == [(2 * per_group, 2 * per_group)] * n


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("order", ["recv_send", "send_recv"])
@pytest.mark.parametrize("mode", ["direct", "scratch"])
def test_sim_asymmetric_grouping(sim_lib, mode, order, seed):
    """DESIGN.md's scenario: rank 0 calls group{send -> 1, recv <- 1}, rank 1 calls recv <- 0 and
    send -> 0 ungrouped, in either order, with a message three times the pair's slots."""
    R = Ranks(2)
    x01, x10 = _bytes(seed, 0, 1, size=LARGEST), _bytes(seed, 1, 0, size=LARGEST)
    d = mode == "direct"
    mine = [[R.recv(1, 0, x01, d)], [R.send(0, x10)]]
    phase = {0: [[R.send(1, x01), R.recv(0, 1, x10, d)]], 1: mine if order == "recv_send" else mine[::-1]}
    _, tx, rx, direct = _run(2, [phase], R, seed)
    assert R.ok()
    tx0, rx0 = _scratch_counters(2, [phase], seed)
    assert np.array_equal(tx, tx0) and np.array_equal(rx, rx0)
    assert direct == [(int(d), int(d))] * 2


def test_sim_direct_ungrouped_sends_need_no_recv_order(sim_lib):
    """What the deadlock rule still says with windows: both ranks send and then receive, ungrouped.  A
    direct send cannot start before its recv posted a destination, so it makes no progress at ANY size
    (the scratch form completes a short one early, which nothing promised)."""
    for size in (SIZES[0], LARGEST):
        R = Ranks(2)
        xs = [_bytes(9, r, size=size) for r in range(2)]
        phase = {r: [[R.send(1 - r, xs[r])], [R.recv(r, 1 - r, xs[1 - r], True)]] for r in range(2)}
        with pytest.raises(RuntimeError):
            _run(2, [phase], R, 0)


def test_sim_count_mismatch_is_refused_before_anything_moves(sim_lib):
    """A send whose byte count differs from its recv's: the sender refuses the record on the direct
    and on the scratch path, and neither arena was written."""
    for direct in (True, False):
        for send_size, recv_size in ((700, 704), (LARGEST, 700)):
            R = Ranks(2)
            x = _bytes(3, size=send_size)
            ph = {0: [[R.send(1, x)]], 1: [[R.recv(1, 0, np.full(recv_size, FILL, np.uint8), direct)]]}
            with pytest.raises(LookupError):
                _run(2, [ph], R, 0)
            assert R.ok()


def test_sim_window_argument_checks(sim_lib):
    R = Ranks(2)
    x = _bytes(1, size=64)
    outside = np.full(64, FILL, np.uint8)
    with pytest.raises(ValueError):  # a recv flagged "in window 0" whose range is not
        _run(2, [{0: [[R.send(1, x)]], 1: [[("recv", 0, outside, 0)]]}], R, 0)
    with pytest.raises(ValueError):  # a window that does not exist
        _run(2, [{0: [[R.send(1, x)]], 1: [[("recv", 0, R.win[1].take(x), 1)]]}], R, 0)
    with pytest.raises(ValueError):  # an unpaired self send is refused as before
        _run(2, [{0: [[("send", 0, x, None)]]}], R, 0)


def test_old_simulator_entry_is_unchanged(sim_lib):
    """mnccl_sim_p2p keeps its signature and runs p2p_kernel's protocol: no DEST word is needed."""
    x, r = _bytes(2, size=LARGEST), np.full(LARGEST + GUARD, FILL, np.uint8)
    P.run(2, [{0: [[("send", 1, x)]], 1: [[("recv", 0, r[:LARGEST])]]}], channels=C, slots=SLOTS, slot_bytes=SLOT, pipes=A)
    assert np.array_equal(r[:LARGEST], x) and (r[LARGEST:] == FILL).all()


# ---------------------------------------------------------------- the pure functions
def test_slot_assignment(sim_lib):
    cap = PW.load().mnccl_p2p_win_slots()
    assert cap == 16
    # lowest free slot; a deregistered slot is handed out again; an unknown id frees nothing
    assert PW.assign([1, 2, 3, -2, 4, 5, -1, -3, 6, 7, -9]) == [0, 1, 2, 1, 1, 3, 0, 2, 0, 2, -1]
    # re-registering the same buffer gets a NEW id (the registration number) and the lowest slot
    assert PW.assign([1, -1, 2]) == [0, 0, 0]
    # a full table: the 17th window has no slot, its deregistration frees nothing, and the next
    # registration after a real deregistration takes the freed slot
    ops = list(range(1, cap + 2)) + [-(cap + 1), -5, cap + 2]
    assert PW.assign(ops) == list(range(cap)) + [-1, -1, 4, 4]


def test_direct_or_scratch_decision(sim_lib):
    L = PW.load()
    assert L.mnccl_p2p_win_direct(1, 0, 1) == 1 and L.mnccl_p2p_win_direct(1, 15, 1) == 1
    assert L.mnccl_p2p_win_direct(0, 0, 1) == 0    # outside every window
    assert L.mnccl_p2p_win_direct(1, -1, 1) == 0   # the window has no table slot (the table was full)
    assert L.mnccl_p2p_win_direct(1, 16, 1) == 0
    assert L.mnccl_p2p_win_direct(1, 0, 0) == 0    # pinned host memory


@pytest.mark.parametrize("tag", [1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 63 + 5, 2 ** 64 - 1])
def test_dest_record_round_trip(sim_lib, tag):
    """Full-width tags (a truncated one would alias across 2^32 messages), offsets and counts."""
    for direct, slot, off, nb in ((1, 0, 0, 2), (1, 15, 2 ** 40 + 6, 2 ** 33 + 2), (0, 0, 0, 2 ** 35), (1, 7, 2, 700)):
        words, back = PW.roundtrip(tag, direct, slot, off, nb)
        assert back == (tag, direct, slot, off, nb)
        assert words[3] == tag and words[1] == off and words[2] == nb
    L = PW.load()
    assert L.mnccl_p2p_dest_tag(tag - 1) == tag  # the counter at the message's start + 1: never 0
    assert PW.roundtrip(2 ** 32 + 1, 1, 0, 0, 2)[0] != PW.roundtrip(1, 1, 0, 0, 2)[0]


def test_dest_record_check(sim_lib):
    L = PW.load()
    ok, bad_bytes, bad_slot, bad_range = 0, 1, 2, 3
    base, wb = 0x7F0000000000, 1 << 20
    assert L.mnccl_p2p_dest_check(1, 3, 4096, 700, 700, base, wb) == ok
    assert L.mnccl_p2p_dest_check(1, 3, wb - 700, 700, 700, base, wb) == ok       # ends exactly at the window's end
    assert L.mnccl_p2p_dest_check(0, 0, 0, 700, 700, 0, 0) == ok                  # scratch: nothing but the count
    # 1. the byte counts differ, on either path
    assert L.mnccl_p2p_dest_check(1, 3, 4096, 704, 700, base, wb) == bad_bytes
    assert L.mnccl_p2p_dest_check(0, 0, 0, 696, 700, 0, 0) == bad_bytes
    # 2. the slot is not valid on this rank: out of range, or free
    assert L.mnccl_p2p_dest_check(1, 16, 0, 700, 700, base, wb) == bad_slot
    assert L.mnccl_p2p_dest_check(1, 3, 0, 700, 700, 0, 0) == bad_slot
    # 3. offset + bytes leaves the window (also where the sum would wrap)
    assert L.mnccl_p2p_dest_check(1, 3, wb - 699, 700, 700, base, wb) == bad_range
    assert L.mnccl_p2p_dest_check(1, 3, wb + 1, 2, 2, base, wb) == bad_range
    assert L.mnccl_p2p_dest_check(1, 3, 2 ** 64 - 4, 700, 700, base, wb) == bad_range


@pytest.mark.parametrize("n,channels", [(2, 2), (3, 256), (8, 256), (16, 64)])
def test_mailbox_layout_grew_behind_abort(sim_lib, n, channels):
    """READY / CREDIT / ABORT keep their offsets; the DEST lines follow, two 16-word lines per
    (receiving rank, pipeline), every word on a line of its own kind."""
    L = PW.load()
    ready, credit, abort, info, tag, words = range(6)
    stride = 16
    for q in (0, n - 1):
        for w in (0, channels - 1):
            assert L.mnccl_mbox_word(ready, n, channels, q, w) == (q * channels + w) * stride
            assert L.mnccl_mbox_word(credit, n, channels, q, w) == (n * channels + q * channels + w) * stride
            i, t = L.mnccl_mbox_word(info, n, channels, q, w), L.mnccl_mbox_word(tag, n, channels, q, w)
            assert i == (2 * n * channels + 1 + 2 * (q * channels + w)) * stride and t == i + stride
    assert L.mnccl_mbox_word(abort, n, channels, 0, 0) == 2 * n * channels * stride
    assert L.mnccl_mbox_word(words, n, channels, 0, 0) == (4 * n * channels + 1) * stride


# ---------------------------------------------------------------- kernel resources
def test_window_kernel_fits_two_waves_per_simd_without_scratch(nccl_lib, tmp_path):
    import re
    all_ks = _kernels(tmp_path)
    ks = {k: v for k, v in all_ks.items() if "p2p_window_group" in k}
    assert len(ks) == 1, sorted(ks)
    for k, v in ks.items():
        assert v["vgpr_count"] + v["agpr_count"] <= 256, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
    # the old kernel is still the only one of its name, and the new name stays out of every existing pattern
    assert len([k for k in all_ks if "p2p_kernel" in k]) == 1
    old = re.compile(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push|"
                     r"varblock_push|collect_push|deal_push|scale_kernel")
    assert not [k for k in ks if old.search(k)]
