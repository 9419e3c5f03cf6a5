"""ctypes front end of ncclCommSplit's host side in the simulator library (csrc/sim.cpp): the plan
(csrc/split.h split_plan, exported as mnccl_split_plan) and the threaded loopback self-test of the
two-round bootstrap (csrc/bootstrap.h split_bootstrap, exported as mnccl_bootstrap_split_selftest).
"""
import ctypes

import sim_api

NOCOLOR = -1
_ready = False


def load():
    global _ready
    L = sim_api.load()
    if not _ready:
        i, P = ctypes.c_int, ctypes.POINTER
        L.mnccl_split_plan.argtypes = [i, P(i), P(i), P(i)]
        L.mnccl_split_plan.restype = None
        L.mnccl_bootstrap_split_selftest.argtypes = [i, i, P(i), P(i), i]
        _ready = True
    return L


def plan(colors, keys):
    """[(group size, new rank, leader's parent rank)] per rank; (0, -1, -1) for a rank in no group."""
    n = len(colors)
    assert len(keys) == n
    c, k = (ctypes.c_int * max(n, 1))(*colors), (ctypes.c_int * max(n, 1))(*keys)
    out = (ctypes.c_int * max(3 * n, 1))()
    load().mnccl_split_plan(n, c, k, out)
    return [tuple(out[3 * r:3 * r + 3]) for r in range(n)]


def plan_restated(colors, keys):
    """The rule in the issue's words: the ranks of one color >= 0, sorted by (key, parent rank)."""
    out = []
    for r, c in enumerate(colors):
        if c < 0:
            out.append((0, -1, -1))
            continue
        members = sorted((keys[q], q) for q in range(len(colors)) if colors[q] == c)
        order = [q for _, q in members]
        out.append((len(order), order.index(r), order[0]))
    return out


def bootstrap_selftest(port, colors, keys, timeout_ms=20000):
    """n ranks as threads over 127.0.0.1:port (see csrc/sim.cpp): 0 on success."""
    n = len(colors)
    c, k = (ctypes.c_int * n)(*colors), (ctypes.c_int * n)(*keys)
    return load().mnccl_bootstrap_split_selftest(n, port, c, k, timeout_ms)
