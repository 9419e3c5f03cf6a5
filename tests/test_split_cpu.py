"""ncclCommSplit without a GPU (-m "not gpu"): the plan (csrc/split.h, through the simulator library's
mnccl_split_plan) against a restatement of the rule, the two-round bootstrap on loopback threads
(mnccl_bootstrap_split_selftest), the ABI's checks that read no communicator, the surface (header,
binding, symbol), and the same host code as a stand-alone program under the sanitizers
(tests/native/split_selftest.cpp).
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sim_split_api as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini-nccl_amd", "csrc")
NOCOLOR = S.NOCOLOR


# ---------------------------------------------------------------- the plan
def _check_plan(colors, keys):
    got = S.plan(colors, keys)
    assert got == S.plan_restated(colors, keys), (colors, keys, got)
    n = len(colors)
    groups = {}
    for r, (size, new, leader) in enumerate(got):
        if colors[r] < 0:
            assert (size, new, leader) == (0, -1, -1), (colors, keys, r)
            continue
        groups.setdefault(colors[r], []).append(r)
        assert colors[leader] == colors[r] and got[leader][1] == 0, (colors, keys, r)  # the leader is new rank 0
    # the groups partition the coloured ranks ...
    assert sorted(r for g in groups.values() for r in g) == [r for r in range(n) if colors[r] >= 0]
    for members in groups.values():
        assert all(got[r][0] == len(members) for r in members)
        # ... and the new ranks are a permutation of 0 ... size - 1, sorted by (key, parent rank)
        by_new = sorted(members, key=lambda r: got[r][1])
        assert [got[r][1] for r in by_new] == list(range(len(members)))
        assert by_new == sorted(members, key=lambda r: (keys[r], r)), (colors, keys)


@pytest.mark.parametrize("n", range(1, 17))
def test_plan_against_the_rule_restated(sim_lib, n):
    """n = 1 ... 16: seeded random colors (some ranks NCCL_SPLIT_NOCOLOR) and keys (negative ones and
    ties), then all-equal keys, negative keys, the extremes of int, every rank NOCOLOR and every rank
    its own color."""
    rng = np.random.default_rng(1000 + n)
    for _ in range(25):
        ncolors = int(rng.integers(1, n + 1))
        colors = [NOCOLOR if rng.integers(0, 5) == 0 else int(rng.integers(0, ncolors)) * 11 for _ in range(n)]
        keys = [int(k) for k in rng.integers(-3, 4, size=n)]
        _check_plan(colors, keys)
    halves = [r % 2 for r in range(n)]
    _check_plan(halves, [5] * n)                       # all-equal keys: the parent's order
    _check_plan(halves, [-r for r in range(n)])        # negative keys: every group reversed
    _check_plan(halves, [-2 ** 31 if r % 3 == 0 else 2 ** 31 - 1 for r in range(n)])
    _check_plan([NOCOLOR] * n, list(range(n)))         # nobody joins
    _check_plan([n - r for r in range(n)], [0] * n)    # every rank its own color
    _check_plan([2 ** 31 - 1] * n, [int(k) for k in rng.integers(-2 ** 31, 2 ** 31, size=n)])


def test_plan_pinned_example(sim_lib):
    """The issue's first GPU case, by hand: 6 ranks, color = rank % 2, key = -rank."""
    got = S.plan([r % 2 for r in range(6)], [-r for r in range(6)])
    assert got == [(3, 2, 4), (3, 2, 5), (3, 1, 4), (3, 1, 5), (3, 0, 4), (3, 0, 5)]
    # ties are broken by the rank in the parent; a NOCOLOR rank is in no group
    assert S.plan([0, NOCOLOR, 0, 0], [1, 0, 1, -7]) == [(3, 1, 3), (0, -1, -1), (3, 2, 3), (3, 0, 3)]


# ---------------------------------------------------------------- the two-round bootstrap
def test_bootstrap_split_on_loopback_threads(sim_lib):
    """5 ranks as threads over 127.0.0.1, colors 0, 1, 0, -1, 1: every child star runs one all-gather
    (the members' parent ranks come back in the plan's order) and one barrier; the parent star still
    works afterwards, and a second split on it (keys negated: every group reversed) works too."""
    import gpu_workers as GW
    assert S.bootstrap_selftest(GW.free_port(), [0, 1, 0, NOCOLOR, 1], [2, -1, 2, 9, -4]) == 0
    # groups of one open no socket; a parent of one rank splits too
    assert S.bootstrap_selftest(GW.free_port(), [3, 2, 1], [0, 0, 0]) == 0
    assert S.bootstrap_selftest(GW.free_port(), [0], [7]) == 0
    assert S.bootstrap_selftest(GW.free_port(), [NOCOLOR, NOCOLOR], [0, 0]) == 0


# ---------------------------------------------------------------- the ABI, no communicator
def test_checks_before_the_communicator_is_read(nccl_lib):
    """Checks 1 - 4 in the header's order with a fake communicator pointer (never dereferenced on these
    paths); *newcomm keeps its value in each."""
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)
    cfg = ctypes.c_void_p(0x2000)
    SENTINEL = 0x5EED5EED
    new = ctypes.c_void_p(SENTINEL)

    def split(comm, color, key, newcomm, config):
        rc = L.ncclCommSplit(comm, color, key, newcomm, config)
        assert new.value == SENTINEL, "a refused ncclCommSplit wrote *newcomm"
        return rc

    # 1. a NULL comm or a NULL newcomm, whatever else is wrong
    assert split(None, 0, 0, ctypes.byref(new), None) == M.ncclInvalidArgument
    assert split(fake, 0, 0, None, None) == M.ncclInvalidArgument
    assert split(None, -5, 0, ctypes.byref(new), cfg) == M.ncclInvalidArgument
    # 2. a group open on this thread, before the config and the color; the group stays open and clean
    with M.group() as g:
        assert split(fake, 0, 0, ctypes.byref(new), None) == M.ncclInvalidUsage
        assert split(fake, -5, 0, ctypes.byref(new), cfg) == M.ncclInvalidUsage
        assert split(None, 0, 0, ctypes.byref(new), None) == M.ncclInvalidArgument  # check 1 still first
    assert g.rc == M.ncclSuccess
    assert L.ncclGroupEnd() == M.ncclInvalidUsage  # ... and is closed now
    # 3. a non-NULL config, before the color
    assert split(fake, 0, 0, ctypes.byref(new), cfg) == M.ncclInvalidUsage
    assert split(fake, -5, 0, ctypes.byref(new), cfg) == M.ncclInvalidUsage
    # 4. a negative color other than NCCL_SPLIT_NOCOLOR
    for color in (-2, -5, -2 ** 31):
        assert split(fake, color, 0, ctypes.byref(new), None) == M.ncclInvalidArgument


# ---------------------------------------------------------------- the surface
def test_surface(nccl_lib):
    import mini_nccl as M
    out = subprocess.run(["nm", "-D", "--defined-only", nccl_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}  # unmangled: C linkage
    assert "ncclCommSplit" in exported
    assert "ncclCommSplit" in M.SIGNATURES and len(M.SIGNATURES["ncclCommSplit"][1]) == 5
    assert M.NCCL_SPLIT_NOCOLOR == -1
    assert callable(M.Comm.split) and callable(M.Comm.split_rc)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, not by version
    with open(os.path.join(ROOT, "include", "mini_nccl_ext.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+NCCL_SPLIT_NOCOLOR\s+\(-1\)", h)
    assert re.search(r"typedef\s+struct\s+ncclConfig\s+ncclConfig_t\s*;", h)
    assert re.search(r"ncclResult_t\s+ncclCommSplit\(ncclComm_t\s+comm,\s*int\s+color,\s*int\s+key,\s*"
                     r"ncclComm_t\*\s*newcomm,\s*ncclConfig_t\*\s*config\);", h)
    assert re.search(r"#define\s+MNCCL_VERSION\s+600\b", h)
    # the concurrency rule is stated where callers read it
    assert "same order" in h[h.index("ncclCommSplit: name"):h.index("#define NCCL_SPLIT_NOCOLOR")]


def test_simulator_exports(sim_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", sim_lib._name], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
    assert {"mnccl_split_plan", "mnccl_bootstrap_split_selftest"} <= exported


# ---------------------------------------------------------------- the host code under the sanitizers
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_split_host_code_under_asan_ubsan(tmp_path):
    """tests/native/split_selftest.cpp: csrc/split.h and csrc/bootstrap.cpp compiled into a stand-alone
    program (its own main, no HIP) with -fsanitize=address,undefined and run as a subprocess: the plan
    over the cases above, the two-round bootstrap, and the leader whose members never connect (a short
    timeout, no descriptor left open).  Nothing is loaded into Python."""
    import gpu_workers as GW
    exe = str(tmp_path / "split_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "native", "split_selftest.cpp"), os.path.join(CSRC, "bootstrap.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(GW.free_port())], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "split selftest: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
