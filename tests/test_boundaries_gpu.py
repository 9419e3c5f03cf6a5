"""The batched fold and push loops at their batch boundaries, the ring's five newer collectives at
n = 2, 5, 8, 9, and a base per rank and buffer (-m gpu): the HIP path through the C ABI, every call
bit for bit against what the other GPU suites compare with -- oracle_api / rooted_ref for the reducing
collectives, the permutation itself for all-gather, broadcast and all-to-all -- with the 256 guard
bytes past recv and last_algo checked per call.

The cases are tests/boundary_cases.py's (one communicator per group, all of its cases on it);
tests/test_boundary_cases.py proves on the CPU that they put the slices on the batch boundaries:
S - 1, S, S + 1 with a sub-vector tail, 2S, 2S + 1 and 3S + 1 vectors for every S = 64 * V of
read_fold_all, copy_push_vec and exchange_push_vec, 1023 ... 1024 + 129 for the fold past
8 ranks, 511 ... 1025 for the ring's move_vec.

The all-reduce's grid form (read_start / read_grid / read_done) runs at MINI_NCCL_GRID_MIN=65536, so a
chunk is 64 KiB and the last workgroup's bytes: 0 (a whole batch of B = 1024 * V), 16, B - 16 and one
vector either side of every row boundary, at n = 2 ... 8, at every V the MINI_NCCL_GRID_VECTORS knob
sets, the whole dtype x op matrix, and bases off 16 bytes; read_grid_calls is checked per call.

Rank r runs on GPU r % ndev, or every rank on GPU 0 on a 1-GPU box (gpu_workers.rank_device): with
the ranks sharing a GPU these tests check the loops' arithmetic and addressing, not cross-device
visibility.
"""
import os

import pytest

import alltoall_workers as AW
import boundary_cases as B
import gpu_workers as GW

pytestmark = pytest.mark.gpu

ENV = {"MINI_NCCL_TIMEOUT_MS": "30000"}
NDEV = [1]


@pytest.fixture(scope="module")
def dev(nccl_lib, oracle_lib):
    # counted in a child: this (pytest) process must hold no GPU queues (gpu_workers.Worker)
    out = GW.run_ranks(GW.device_count_probe, 1, lambda r: (), 120)
    if not out or out[0]["count"] < 1:
        pytest.fail("no HIP device visible: the -m gpu suite must run on the MI355X box")
    NDEV[0] = out[0]["count"]
    return NDEV[0]


def _run_group(name, timeout=300):
    g = B.GROUPS[name]
    n, cases, port = g["n"], g["cases"], GW.free_port()
    e = dict(ENV, **g["env"])
    out = GW.run_ranks(AW.a2a_rank, n, lambda r: (r, n, port, cases, e), timeout, barrier=True)
    assert sorted(out) == list(range(n)), f"only ranks {sorted(out)} reported (timeout?)"
    colo = GW.colocated(dict(os.environ, **e))
    for r in range(n):
        assert "error" not in out[r], f"rank {r}:\n{out[r]['error']}"
        assert out[r]["destroy"] == 0
        assert out[r]["info"]["device"] == GW.rank_device(r, NDEV[0], colo), (r, out[r]["info"]["device"])
        assert out[r]["info"]["ranks_on_device"] == GW.ranks_sharing_device(r, n, NDEV[0], colo), (r, n, NDEV[0])
        assert len(out[r]["results"]) == len(cases)
        for res in out[r]["results"]:
            c = res["case"]
            assert res["rc"] == 0, f"rank {r} case {c}: ncclResult {res['rc']}"
            assert res["bad"] == 0, f"rank {r} case {c}: {res['bad']} mismatches, first at {res['first']} {res['detail']}"
            assert res["async"] == 0
            assert res["ipc_open_failures"] == 0 and res["read_map_failures"] == 0, (r, c, res)
            # device buffers: the read schedule where it is asked for (the element path too), else the ring
            # (expect_algo: what a forced grid or auto call reports -- the read schedule)
            assert res["algos"] == [c.get("expect_algo", c["algo"])], f"rank {r} case {c}: ran schedules {res['algos']}"
            if "expect_grid" in c:
                assert res["grid_calls"] == (1 if c["expect_grid"] else 0), f"rank {r} case {c}: {res['grid_calls']} grid-form calls"
    return out


@pytest.mark.parametrize("n", B.READ_NS)
def test_read_batch_boundaries(dev, n):
    """One pipeline, so the chunk's last slice is the class: every class of the fold (reduce-scatter,
    all-reduce, reduce: f32 and bf16 sum, f64 max and f16 prod at S + 1 with a tail) and of the pushes
    (all-gather, broadcast with roots 0 and n - 1, all-to-all with 1536 vectors too), out of place and
    in place, a non-root passing NULL in half the rooted cases, count = n * q and the clamped last chunk."""
    _run_group(f"read-n{n}")


@pytest.mark.parametrize("n", B.ROT_NS)
def test_read_ragged_batches_on_four_pipelines(dev, n):
    """Slices of 513 vectors on 4 pipelines (two and three iterations): the pushes start at destination
    w mod (n - 1) while the batch parity carries across destinations and iterations."""
    _run_group(f"rot-n{n}")


@pytest.mark.parametrize("n", B.RING_NS)
def test_ring_small_slices(dev, n):
    """The ring's op tables of the five newer collectives at n = 2, 5, 8, 9 with 1 KiB slices on 4
    pipelines over 2 slots: up to 17 iterations per pipeline, roots 0 and n - 1."""
    _run_group(f"ring-small-n{n}")


def test_ring_default_geometry_move_vec_boundaries(dev):
    """n = 5 at the default geometry: 256 messages per op whose lengths put move_vec on 511, 512,
    513 (with a tail), 1024 and 1025 vectors."""
    _run_group(f"ring-default-n{B.RING_DEFAULT_N}")


@pytest.mark.parametrize("n", B.ALIGN_NS)
def test_base_per_rank_and_buffer(dev, n):
    """Rank r's send 4 * (r mod 4) and its recv 4 * ((r + 1) mod 4) bytes into their allocations (the
    vector path, every rank and buffer on another 16-byte phase), and rank 1 alone 2-byte-misaligned
    with bf16 (the element path on every rank of the read schedule): every collective, read and ring."""
    _run_group(f"align-n{n}")


@pytest.mark.parametrize("n", B.GRID_NS)
def test_grid_batch_boundaries(dev, n):
    """The all-reduce's grid form at every rank count it has (G = 1, 2, 4, 4, 7, 7, 7 peer slots, the
    last two masked at n = 6 and 7), chunks of 64 KiB and a last workgroup of every class of the
    rule's V: f32 and bf16 sum out of place and in place with and without a tail, the 5 x 4 dtype x op
    matrix one vector into the last row, and the calls either side of the threshold, forced and auto,
    so that grid and persistent calls follow each other on one communicator."""
    _run_group(f"grid-n{n}")


@pytest.mark.parametrize("n,vectors", [(n, v) for n in B.GRID_NS for v in B.GRID_VS if v != B.grid_rule_v(n)])
def test_grid_vectors_batch_boundaries(dev, n, vectors):
    """MINI_NCCL_GRID_VECTORS off the rule: f32 sum at every class of the knob's V (the host's grid
    and the kernel's template argument must agree on it), f32 prod and bf16 sum on the rule's."""
    _run_group(f"grid-v-n{n}-v{vectors}")


@pytest.mark.parametrize("n", B.GRID_ALIGN_NS)
def test_grid_bases_off_16_bytes(dev, n):
    """The grid form with rank r's send 4 * (r mod 4) and its recv 4 * ((r + 1) mod 4) bytes into
    their allocations; rank 1 alone 2-byte-misaligned with bf16 runs the persistent kernel's element
    path instead."""
    _run_group(f"grid-align-n{n}")
