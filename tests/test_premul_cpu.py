"""ncclRedOpCreatePreMulSum / ncclRedOpDestroy without a GPU (-m "not gpu"): the symbols and enum
values, the checks that return before any device work, the binding, the numpy reference the GPU
tests compare against (tests/premul_ref.py) pinned on hand-computed values, the GPU tests' inputs
(able to see a contracted multiply-add), and the resource budget of the new kernels.
"""
import ctypes
import os
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import premul_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_H = os.path.join(ROOT, "include", "mini_nccl_ext.h")


# ---------------------------------------------------------------- the interface
def test_symbols_and_enum_values(nccl_lib):
    import mini_nccl as M
    assert nccl_lib.ncclRedOpCreatePreMulSum is not None and nccl_lib.ncclRedOpDestroy is not None
    assert (M.ncclScalarDevice, M.ncclScalarHostImmediate) == (0, 1)
    assert M.MNCCL_FIRST_USER_OP == 5 == M.ncclAvg + 1
    hdr = open(EXT_H).read()
    assert re.search(r"typedef enum \{ ncclScalarDevice = 0, ncclScalarHostImmediate = 1 \} ncclScalarResidence_t;", hdr)
    assert re.search(r"#define MNCCL_FIRST_USER_OP 5\b", hdr)
    # NCCL's names and argument order
    assert re.search(r"ncclResult_t ncclRedOpCreatePreMulSum\(ncclRedOp_t\* op, void\* scalar, ncclDataType_t datatype,\s+"
                     r"ncclScalarResidence_t residence, ncclComm_t comm\);", hdr)
    assert re.search(r"ncclResult_t ncclRedOpDestroy\(ncclRedOp_t op, ncclComm_t comm\);", hdr)
    assert nccl_lib.mncclVersion() == 600  # detected by symbol, as everything since 600


def test_null_checks_come_first(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced on these paths
    op = ctypes.c_int(-1)
    one = ctypes.c_float(1.0)
    sc = ctypes.cast(ctypes.byref(one), ctypes.c_void_p)
    host = M.ncclScalarHostImmediate
    assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), sc, M.ncclFloat, host, None) == M.ncclInvalidArgument
    assert L.ncclRedOpCreatePreMulSum(None, sc, M.ncclFloat, host, fake) == M.ncclInvalidArgument
    assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), None, M.ncclFloat, host, fake) == M.ncclInvalidArgument
    # a NULL argument wins over an unsupported datatype, and that over anything read from the communicator
    assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), None, M.ncclInt8, host, fake) == M.ncclInvalidArgument
    for dt in (M.ncclInt8, M.ncclUint8, M.ncclUint32, M.ncclInt64, M.ncclUint64):
        assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), sc, dt, host, fake) == M.ncclInternalError
    assert op.value == -1  # nothing was written
    assert L.ncclRedOpDestroy(M.MNCCL_FIRST_USER_OP, None) == M.ncclInvalidArgument
    assert L.ncclRedOpDestroy(M.ncclSum, None) == M.ncclInvalidArgument


def test_builtin_ops_are_checked_before_the_communicator_is_read(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)
    # ncclAvg and a negative op never reach the communicator (a fake pointer here): ncclInternalError
    for bad in (M.ncclAvg, -1):
        assert L.ncclAllReduce(fake, fake, 4, M.ncclFloat, bad, fake, None) == M.ncclInternalError
        assert L.ncclReduceScatter(fake, fake, 4, M.ncclFloat, bad, fake, None) == M.ncclInternalError
        assert L.ncclReduce(fake, fake, 4, M.ncclFloat, bad, 0, fake, None) == M.ncclInternalError
    # an unsupported datatype wins over a user op's lookup
    assert L.ncclAllReduce(fake, fake, 4, M.ncclInt8, M.MNCCL_FIRST_USER_OP, fake, None) == M.ncclInternalError
    # the count == 0 rule and the NULL checks come before the op, as for every op
    assert L.ncclAllReduce(fake, fake, 0, M.ncclFloat, M.MNCCL_FIRST_USER_OP, fake, None) == M.ncclSuccess
    assert L.ncclAllReduce(None, fake, 4, M.ncclFloat, M.MNCCL_FIRST_USER_OP, fake, None) == M.ncclInvalidArgument
    # mncclLocalReduce has no communicator: the four built-ins only
    for bad in (M.ncclAvg, M.MNCCL_FIRST_USER_OP, M.MNCCL_FIRST_USER_OP + 3):
        assert L.mncclLocalReduce(fake, fake, fake, 4, M.ncclFloat, bad, None) == M.ncclInternalError


def test_binding_round_trip(nccl_lib):
    import mini_nccl as M
    assert M.SIGNATURES["ncclRedOpCreatePreMulSum"][1][2:4] == [ctypes.c_int, ctypes.c_int]
    assert callable(M.Comm.redop_premul_sum) and callable(M.Comm.redop_destroy) and callable(M.Comm.redop_premul_sum_rc)
    # the scalar's bytes, one value of the datatype in little-endian order
    assert M.scalar_bytes(0.3, M.ncclFloat).raw[:4] == struct.pack("<f", 0.3)
    assert M.scalar_bytes(-2.5, M.ncclDouble).raw[:8] == struct.pack("<d", -2.5)
    assert M.scalar_bytes(-7, M.ncclInt32).raw[:4] == struct.pack("<i", -7)
    assert M.scalar_bytes(0.3, M.ncclFloat16).raw[:2] == np.float16(0.3).tobytes()
    assert M.scalar_bytes(0.3, M.ncclBfloat16).raw[:2] == struct.pack("<H", 0x3E9A)  # 0.30078125
    assert M.scalar_bytes(0x3E9A, M.ncclBfloat16).raw[:2] == struct.pack("<H", 0x3E9A)
    assert M.scalar_bytes(np.uint16(0x3E9A), M.ncclBfloat16).raw[:2] == struct.pack("<H", 0x3E9A)  # the bits, any integer type
    assert M.scalar_bytes(np.float32(0.3), M.ncclBfloat16).raw[:2] == struct.pack("<H", 0x3E9A)
    assert M.scalar_bytes(np.float16(0.3), M.ncclFloat16).raw[:2] == np.float16(0.3).tobytes()
    # through a Comm object without a communicator behind it: the library's NULL check answers
    c = M.Comm.__new__(M.Comm)
    c.handle = ctypes.c_void_p()
    assert c.redop_premul_sum_rc(0.5, M.ncclFloat) == (M.ncclInvalidArgument, -1)
    assert c.redop_destroy(M.MNCCL_FIRST_USER_OP) == M.ncclInvalidArgument
    with pytest.raises(M.NcclError):
        c.redop_premul_sum(0.5, M.ncclFloat)
    # what the tests hand to the binding is the reference's scalar
    for dt in P.DTYPES:
        for s in P.scalars(dt, 3):
            import oracle_api as O
            raw = M.scalar_bytes(P.scalar_arg(s, dt), O.DTYPES[dt][0]).raw
            assert raw[:np.dtype(O.DTYPES[dt][1]).itemsize] == P.scalar_value(s, dt).tobytes(), (dt, s)


# ---------------------------------------------------------------- the reference, hand-computed
def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)


def test_prescale_reference_on_hand_computed_values():
    # f32: (1 + 2^-23)^2 = 1 + 2^-22 + 2^-46 -> 1 + 2^-22; 1.5 * (1 + 2^-23) = 1.5 + 2^-23 + 2^-24, a tie
    # between 0x3FC00001 (odd) and 0x3FC00002 (even); 1.5 * (1 + 3 * 2^-23) ties down to 0x3FC00004
    assert P.prescale(_f32(0x3F800001), float(_f32(0x3F800001)[0]), "f32").view(np.uint32)[0] == 0x3F800002
    assert P.prescale(_f32(0x3F800001), 1.5, "f32").view(np.uint32)[0] == 0x3FC00002
    assert P.prescale(_f32(0x3F800003), 1.5, "f32").view(np.uint32)[0] == 0x3FC00004
    assert P.prescale(np.array([3.0, -0.5], np.float32), -2.5, "f32").tolist() == [-7.5, 1.25]
    # f64: the same tie one format up
    x = np.array([0x3FF0000000000001], np.uint64).view(np.float64)
    assert P.prescale(x, 1.5, "f64").view(np.uint64)[0] == 0x3FF8000000000002
    # f16 (10 fraction bits): 1.5 * (1 + 2^-10) = 1.5 + 2^-10 + 2^-11: a tie, up to the even 0x3E02;
    # 1.5 * (1 + 3 * 2^-10) = 1.5 + 4 * 2^-10 + 2^-11: a tie, down to the even 0x3E04
    h = np.array([0x3C01, 0x3C03], np.uint16).view(np.float16)
    assert P.prescale(h, 1.5, "f16").view(np.uint16).tolist() == [0x3E02, 0x3E04]
    # bf16 (7 fraction bits): 1.5 * (1 + 2^-7) = 1.5 + 2^-7 + 2^-8: a tie, up to the even 0x3FC2;
    # 1.5 * (1 + 3 * 2^-7): a tie, down to the even 0x3FC4; and 0.3 is the bf16 0x3E9A = 0.30078125,
    # times 2.0 exactly 0x3F1A
    b = np.array([0x3F81, 0x3F83], np.uint16)
    assert P.prescale(b, 1.5, "bf16").tolist() == [0x3FC2, 0x3FC4]
    assert int(P.scalar_value(0.3, "bf16")) == 0x3E9A
    assert P.prescale(np.array([0x4000], np.uint16), 0.3, "bf16").tolist() == [0x3F1A]
    # i32 wraps: 3 * (2^31 - 1) = 2^32 + 2^31 - 3 -> 2^31 - 3; 3 * -2^31 = -2^32 - 2^31 -> -2^31;
    # -7 * (2^31 - 1) = -8 * 2^31 + 2^31 + 7 -> 2^31 + 7 -> -2^31 + 7; -7 * -2^31 = 6 * 2^31 + 2^31 -> -2^31
    i = np.array([0x7FFFFFFF, -2 ** 31, 3], np.int64).astype(np.int32)
    assert P.prescale(i, 3, "i32").tolist() == [2 ** 31 - 3, -2 ** 31, 9]
    assert P.prescale(i, -7, "i32").tolist() == [-2 ** 31 + 7, -2 ** 31, -21]


def test_exact_rounding_helper():
    # round_fraction is the yardstick of the contraction check below: held against numpy's own casts
    g = np.random.default_rng(5)
    for v in g.uniform(-4, 4, 200):
        fr = Fraction(float(v))
        assert P.round_fraction(fr, "f32") == Fraction(float(np.float32(v)))
        assert P.round_fraction(fr, "f16") == Fraction(float(np.float16(v)))
        import oracle_api as O
        assert P.round_fraction(Fraction(float(np.float32(v))), "bf16") == \
            Fraction(float(O.bf16_to_f32(O.bf16_from_f32(np.array([v], np.float32)))[0]))
    assert P.round_fraction(Fraction(3, 2) + Fraction(1, 2 ** 24), "f32") == Fraction(3, 2)  # a tie, to even
    assert P.round_fraction(Fraction(1, 3), "f64") == Fraction(1.0 / 3.0)


def test_all_reduce_expectation_keeps_the_raw_tail(oracle_lib):
    import oracle_api as O
    n, count = 3, 3 * 5 + 2
    xs = P.inputs(n, count, "f32", 1)
    for r in range(n):
        e = P.allreduce_expect(xs, 0.3, "f32", r)
        assert np.array_equal(e[15:], xs[r][15:])
        body = O.ring_fold([P.prescale(x, 0.3, "f32") for x in xs], "f32", "sum")[:15]
        assert np.array_equal(e[:15].view(np.uint32), body.view(np.uint32))
    assert np.array_equal(P.reduce_scatter_expect(xs[0:3], 0.3, "f32", 1).view(np.uint32),
                          O.ring_fold([P.prescale(x, 0.3, "f32") for x in xs], "f32", "sum")[5:10].view(np.uint32))


# ---------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("n", [2, 3, 5, 8, 9])
def test_gpu_inputs_can_see_a_contracted_multiply_add(n):
    """For every float datatype and scalar of the parity cases at n ranks there is a case whose
    inputs hold an element where round(s * x + acc) differs from round(round(s * x) + acc) at the
    fold's first step (chunk 0: acc = y_0, then y_1 + acc), the fused value computed exactly."""
    seen = {}
    for case in P.parity_cases(n):
        dt, s = case["dtype"], case["s"]
        if dt not in P.FLOATS or seen.get((dt, s), -1) >= 0:
            continue
        count = n * case["chunk"] + case["tail"]
        xs = P.inputs(n, count, dt, case["seed"])
        c = case["chunk"]
        seen[(dt, s)] = P.fused_differs(xs[0][:c], xs[1][:c], s, dt, limit=512)
    want = {(dt, s) for dt in P.parity_dtypes(n) if dt in P.FLOATS for s in P.scalars(dt, n)}
    assert set(seen) == want
    # (a power of two -- 1 / n at 2 and 8 ranks -- scales exactly: fused or not, the bits are the
    # same, and no input could tell; every datatype keeps 0.3 and -2.5, which do round)
    import math
    blind = {k: v for k, v in seen.items() if v < 0 and math.frexp(k[1])[0] != 0.5}
    assert not blind, f"inputs that could not show a fused multiply-add: {blind}"
    assert all(sum(1 for (dt, s), v in seen.items() if dt == d and v >= 0) >= 2 for d in {k[0] for k in seen})


def test_parity_cases_cover_what_they_claim():
    import boundary_cases as BC
    for n in (2, 3, 5, 8, 9):
        cases = P.parity_cases(n)
        got = {(c["dtype"], c["s"], c["coll"], c["algo"]) for c in cases}
        want = {(dt, s, coll, algo) for dt in P.parity_dtypes(n) for s in P.scalars(dt, n) for coll in ("ar", "rs", "rd")
                for algo in (P.RING, P.READ)}
        assert got == want, (n, sorted(want - got))
        assert {c["inplace"] for c in cases} == {False, True}
        assert len({c["seed"] for c in cases}) == len(cases)
        for dt in P.parity_dtypes(n):
            esz = BC.ESZ[dt]
            cb = P.shape_b_chunk(n, dt) * esz
            # under ONE the chunk's last (or only) slice: two full batches, 5 vectors, one element
            last = cb if cb <= 16384 else cb - 15 * ((cb // 16 + 1023) // 1024 * 1024)
            assert last == (2 * BC.fold_batch(n, esz) + 5) * 16 + esz, (n, dt, cb, last)
    # the fold's batches as the kernel states them (kernels.hip read_fold: G peer slots, V vectors)
    src = open(os.path.join(ROOT, "mini-nccl_amd", "csrc", "kernels.hip")).read()
    for pat in (r"n == 2\) read_fold_all<T, OPC, 1, 12 - 4 \* h, PUSH>", r"n == 3\) read_fold_all<T, OPC, 2, 8 - 2 \* h, PUSH>",
                r"n <= 5\) read_fold_all<T, OPC, 4, 4 - h, PUSH>", r"else read_fold_all<T, OPC, 7, 3 - h, PUSH>",
                r"constexpr int h = sizeof\(T\) == 2 \? 1 : 0;", r"#define MNCCL_READ_FOLD_U 16"):
        assert re.search(pat, src), pat
    assert [BC.fold_batch(n, 4) for n in (2, 3, 5, 8, 9)] == [64 * 12, 64 * 8, 64 * 4, 64 * 3, 64 * 16]
    assert [BC.fold_batch(n, 2) for n in (2, 3, 5, 8)] == [64 * 8, 64 * 6, 64 * 3, 64 * 2]


# ---------------------------------------------------------------- the new kernels' budget
def test_scaled_kernels_fit_two_waves_per_simd_without_scratch(tmp_path):
    """tests/test_kernel_resources.py's check for the entry points its name filter does not see: the
    scaled_* kernels (the persistent kernels of a pre-multiplied sum) stay within 256 registers per
    lane and use no scratch memory, as every kernel of the library."""
    import test_kernel_resources as R
    if not (os.path.exists(R.LIB) and os.path.exists(R.READELF)):
        pytest.skip("library not built / no llvm-readelf")
    ks = R._kernels(tmp_path)
    scaled = {k: v for k, v in ks.items() if re.search(r"scaled_(ring|read|scatter|root)", k)}
    # (ring, read, scatter, root) x 5 datatypes x (vector, scalar)
    assert len(scaled) == 4 * 10, sorted(scaled)
    # none of them is counted by the existing filter (whose exact count must stay what it was)
    assert not [k for k in scaled if re.search(r"(ring|read|oneshot)_kernel|scatter_fold|root_fold", k)]
    over = {k: v for k, v in scaled.items() if v["vgpr_count"] + v["agpr_count"] > 256}
    assert not over, f"scaled kernels above 256 registers: {over}"
    spill = {k: v for k, v in ks.items() if v["private_segment_fixed_size"] != 0}
    assert not spill, f"kernels using scratch memory: {spill}"
    # the grid form's and the one-rank scale kernel's instantiations exist too
    assert len([k for k in ks if re.search(r"read_grid_kernelI\w+Li5E", k)]) == 5 * 5
    assert len([k for k in ks if "scale_kernel" in k]) == 5
