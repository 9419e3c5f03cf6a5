"""The fp8 datatypes (ncclFloat8e4m3 / ncclFloat8e5m2) without a GPU (-m "not gpu"): the numpy
reference the GPU tests compare against (tests/fp8_ref.py) held against torch's CPU fp8 casts and
against the contract's rules stated directly, the checks of the C ABI that return before any device
work, the binding, and the new kernels as built: their resource budget, their exact number, their
names, and the packed conversions in their vector paths.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import fp8_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_H = os.path.join(ROOT, "include", "mini_nccl_ext.h")


def _torch_dtype(fmt):
    import torch
    return {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[fmt]


def _torch_cast(x, fmt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(_torch_dtype(fmt)).view(torch.uint8).numpy()


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("fmt", list(F.FORMATS))
def test_decode_equals_torch_on_all_codes(fmt):
    import torch
    t = torch.arange(256, dtype=torch.uint8).view(_torch_dtype(fmt)).float().numpy()
    d = F.decode_table(fmt)
    ok = ~np.isnan(t)
    assert np.array_equal(np.isnan(t), np.isnan(d))
    assert np.array_equal(t[ok].view(np.uint32), d[ok].view(np.uint32))  # values, infinities, the sign of zero


def test_the_encodings_are_ocp():
    d4, d5 = F.decode_table("e4m3"), F.decode_table("e5m2")
    assert F.max_code("e4m3") == 0x7E and d4[0x7E] == 448 and d4[0xFE] == -448
    assert np.flatnonzero(np.isnan(d4)).tolist() == [0x7F, 0xFF] and not np.isinf(d4).any()
    assert d4[0x01] == 2.0 ** -9 and d4[0x08] == 2.0 ** -6 and d4[0x38] == 1.0
    assert F.max_code("e5m2") == 0x7B and d5[0x7B] == 57344 and d5[0xFB] == -57344
    assert d5[0x7C] == np.inf and d5[0xFC] == -np.inf
    assert np.flatnonzero(np.isnan(d5)).tolist() == [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]
    assert d5[0x01] == 2.0 ** -16 and d5[0x04] == 2.0 ** -14 and d5[0x3C] == 1.0
    assert d4[0x80] == 0 and np.signbit(d4[0x80]) and d5[0x80] == 0 and np.signbit(d5[0x80])  # (not fnuz's NaN)


def _neighbours(v):
    """Each float32 with the one below and the one above it."""
    v = np.asarray(v, np.float32)
    return np.unique(np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]))


@pytest.mark.parametrize("fmt", list(F.FORMATS))
def test_encode_equals_torch_on_the_grid_its_midpoints_and_their_neighbours(fmt):
    d = F.decode_table(fmt)
    pos = np.sort(d[np.isfinite(d) & ~np.signbit(d)])
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(np.float32)  # exact in float32
    assert np.array_equal(mid.astype(np.float64) * 2, pos[:-1].astype(np.float64) + pos[1:])
    x = _neighbours(np.concatenate([pos, mid]))
    x = x[np.abs(x) <= F.max_finite(fmt)]                 # in range: torch does not saturate beyond
    x = np.concatenate([x, -x])
    assert x.size > 6 * pos.size
    assert np.array_equal(F.encode(x, fmt), _torch_cast(x, fmt))
    # and a few hundred thousand random values over the whole range, subnormals included
    g = np.random.default_rng(3)
    r = (g.uniform(-1, 1, 200000) * F.max_finite(fmt) * g.choice([1, 1e-2, 1e-4, 1e-6], 200000)).astype(np.float32)
    assert np.array_equal(F.encode(r, fmt), _torch_cast(r, fmt))


@pytest.mark.parametrize("fmt", list(F.FORMATS))
def test_round_trips(fmt):
    codes = np.arange(256, dtype=np.uint8)
    back = F.encode(F.decode(codes, fmt), fmt)
    nan = F.is_nan(codes, fmt)
    assert np.array_equal(back[~nan], codes[~nan])        # every finite code, both zeros, e5m2's infinities
    assert F.is_nan(back[nan], fmt).all()


def test_saturation_inf_and_nan_rules():
    f32 = lambda *v: np.array(v, np.float32)
    # e4m3: the grid's step at 448 is 32, so 464 is the midpoint to the (absent) 480: everything finite
    # beyond 448 saturates, the largest float32 included; never inf, never NaN
    assert F.encode(f32(448, 463.9, 464, 464.1, 480, 1e9, 3.4028235e38), "e4m3").tolist() == [0x7E] * 7
    assert F.encode(f32(-448, -464, -1e9), "e4m3").tolist() == [0xFE] * 3
    assert F.is_nan(F.encode(f32(np.nan, -np.nan), "e4m3"), "e4m3").all()
    # e5m2: step 8192 at 57344, midpoint 61440 to the (absent) 65536
    assert F.encode(f32(57344, 61439, 61440, 61441, 65536, 1e9, 3.4028235e38), "e5m2").tolist() == [0x7B] * 7
    assert F.encode(f32(-57344, -61440, -1e9), "e5m2").tolist() == [0xFB] * 3
    assert F.encode(f32(np.inf, -np.inf), "e5m2").tolist() == [0x7C, 0xFC]
    assert F.is_nan(F.encode(f32(np.nan), "e5m2"), "e5m2").all()
    # saturation is reported for finite values only, and only where the rounded value left the grid
    assert F.encode_flags(f32(448, 463, 465, np.nan), "e4m3")[1].tolist() == [False, False, True, False]
    assert F.encode_flags(f32(57344, 61439, 61441, np.inf, np.nan), "e5m2")[1].tolist() == [False, False, True, False, False]
    # subnormals round to nearest even, the sign of zero is kept
    assert F.encode(f32(2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 2.0 ** -11), "e4m3").tolist() == [1, 0, 2, 2, 0]
    assert F.encode(f32(-0.0, 0.0, -(2.0 ** -11)), "e4m3").tolist() == [0x80, 0x00, 0x80]
    assert F.encode(f32(2.0 ** -16, 2.0 ** -17, 1.5 * 2.0 ** -16, -0.0), "e5m2").tolist() == [1, 0, 2, 0x80]


def test_fold_rules():
    u8 = lambda *v: np.array(v, np.uint8)
    # e4m3: 448 + 448 saturates; 448 * 448 saturates; 1 + 2^-9 -> 1 (one rounding); 1.125 * 1.125 = 1.265625 -> 1.25
    assert F.fold(u8(0x7E, 0x7E, 0x38, 0x39), u8(0x7E, 0xFE, 0x01, 0x39), "e4m3", "sum").tolist() == [0x7E, 0x00, 0x38, 0x41]
    assert F.fold(u8(0x7E, 0x39), u8(0x7E, 0x39), "e4m3", "prod").tolist() == [0x7E, 0x3A]
    stats = {}
    F.fold(u8(0x7E, 0x38), u8(0x7E, 0x38), "e4m3", "sum", stats)
    assert stats == {"sat": 1, "nan": 0}
    # e5m2: inf + finite = inf, inf - inf = NaN, 57344 + 57344 saturates and does not become inf
    out = F.fold(u8(0x7C, 0x7C, 0x7B), u8(0x3C, 0xFC, 0x7B), "e5m2", "sum")
    assert out[0] == 0x7C and F.is_nan(out[1:2], "e5m2").all() and out[2] == 0x7B
    # Max / Min: (fa > fb) ? a : b -- a NaN on either side gives the INCOMING operand b; equal values
    # (+0 and -0) give b; an operand's byte comes back unchanged
    a, b = u8(0x7F, 0x38, 0x00, 0x80, 0x40), u8(0x38, 0x7F, 0x80, 0x00, 0x38)
    assert F.fold(a, b, "e4m3", "max").tolist() == [0x38, 0x7F, 0x80, 0x00, 0x40]
    assert F.fold(a, b, "e4m3", "min").tolist() == [0x38, 0x7F, 0x80, 0x00, 0x38]
    # the scale: one product, one rounding, saturating
    assert F.scale(u8(0x38, 0x7E), 0x40, "e4m3").tolist() == [0x40, 0x7E]  # 2 * 1 = 2; 2 * 448 saturates


def test_association_tail_and_rooted_partition():
    n, fmt = 3, "e4m3"
    xs = F.inputs(n, 3 * 5 + 2, fmt, 1, "plain")
    body = F.ring_fold(xs, fmt, "sum")
    assert body.size == 15
    for c in range(n):   # chunk c: acc = x_c, then op(x_q, acc) for q = c + 1, c + 2
        acc = xs[c][5 * c:5 * c + 5]
        for k in (1, 2):
            acc = F.fold(xs[(c + k) % n][5 * c:5 * c + 5], acc, fmt, "sum")
        assert np.array_equal(body[5 * c:5 * c + 5], acc)
    for r in range(n):
        e = F.allreduce_expect(xs, fmt, "sum", r)
        assert np.array_equal(e[:15], body) and np.array_equal(e[15:], xs[r][15:])  # the raw tail
        assert np.array_equal(F.reduce_scatter_expect(xs[:], fmt, "sum", r), F.ring_fold([x[:15] for x in xs], fmt, "sum")[5 * r:5 * r + 5])
    # ncclReduce: chunks of ceil(17 / 3) = 6, 6 and 5 elements, no tail
    rd = F.reduce_expect(xs, fmt, "max")
    for c, (lo, hi) in enumerate(((0, 6), (6, 12), (12, 17))):
        acc = xs[c][lo:hi]
        for k in (1, 2):
            acc = F.fold(xs[(c + k) % n][lo:hi], acc, fmt, "max")
        assert np.array_equal(rd[lo:hi], acc)
    # a pre-multiplied sum scales every input on its way in, and the all-reduce's tail stays unscaled
    s = 0x34
    e = F.allreduce_expect(xs, fmt, "premul", 1, s)
    assert np.array_equal(e[:15], F.ring_fold([F.scale(x, s, fmt) for x in xs], fmt, "sum")) and np.array_equal(e[15:], xs[1][15:])


def test_plain_inputs_stay_clear_of_nan_and_saturation():
    for fmt in F.FORMATS:
        v = F.decode(F.plain_codes(fmt), fmt)
        assert np.isfinite(v).all() and np.abs(v).max() < 8 and F.plain_codes(fmt).size > 100
        assert 8 * np.abs(v).max() < F.max_finite(fmt) and np.abs(v).max() ** 3 < F.max_finite(fmt)
    assert F.mismatches(np.array([0x7F, 0x7E], np.uint8), np.array([0xFF, 0x7E], np.uint8), "e4m3") == (0, -1)
    assert F.mismatches(np.array([0x7F, 0x7E], np.uint8), np.array([0x7E, 0x7E], np.uint8), "e4m3") == (1, 0)
    assert F.mismatches(np.array([0x7C], np.uint8), np.array([0x7D], np.uint8), "e5m2") == (1, 0)  # inf is no NaN


# ---------------------------------------------------------------- the C ABI, before any device work
def test_header_and_symbols(nccl_lib):
    import mini_nccl as M
    hdr = open(EXT_H).read()
    assert re.search(r"#define ncclFloat8e4m3 \(\(ncclDataType_t\)10\)", hdr)
    assert re.search(r"#define ncclFloat8e5m2 \(\(ncclDataType_t\)11\)", hdr)
    assert re.search(r"ncclResult_t mncclDataTypeSize\(ncclDataType_t datatype, size_t\* size\);", hdr)
    assert (M.ncclFloat8e4m3, M.ncclFloat8e5m2) == (10, 11) == (F.code("e4m3"), F.code("e5m2"))
    assert M.DTYPE_SIZE[M.ncclFloat8e4m3] == 1 and M.DTYPE_SIZE[M.ncclFloat8e5m2] == 1
    assert "mncclDataTypeSize" in M.SIGNATURES and nccl_lib.mncclDataTypeSize is not None
    assert nccl_lib.mncclVersion() == 600  # detected by symbol


def test_data_type_size(nccl_lib):
    import mini_nccl as M
    for dt, size in ((10, 1), (11, 1), (M.ncclInt32, 4), (M.ncclFloat16, 2), (M.ncclFloat, 4), (M.ncclDouble, 8),
                     (M.ncclBfloat16, 2)):
        assert M.data_type_size(dt) == (M.ncclSuccess, size) == (0, M.DTYPE_SIZE[dt])
    n = ctypes.c_size_t(77)
    for bad in (0, 1, 3, 4, 5, 12, 255, -1):
        assert nccl_lib.mncclDataTypeSize(bad, ctypes.byref(n)) == M.ncclInvalidArgument
        assert n.value == 77  # untouched
    assert nccl_lib.mncclDataTypeSize(10, None) == M.ncclInvalidArgument
    assert nccl_lib.mncclDataTypeSize(0, None) == M.ncclInvalidArgument


FOLDING = ("ncclAllReduce", "ncclReduceScatter", "ncclReduce", "mncclLocalReduce")


def _calls(L, fake, count, dt, op, movers=True):
    """The calls of the ABI that take a datatype, on fake pointers: {name: ncclResult_t}.  Only for
    arguments a call answers before it reads its communicator (movers=False: the folding calls alone,
    whose op check does so too)."""
    res = {
        "ncclAllReduce": L.ncclAllReduce(fake, fake, count, dt, op, fake, None),
        "ncclReduceScatter": L.ncclReduceScatter(fake, fake, count, dt, op, fake, None),
        "ncclReduce": L.ncclReduce(fake, fake, count, dt, op, 0, fake, None),
        "mncclLocalReduce": L.mncclLocalReduce(fake, fake, fake, count, dt, op, None),
    }
    if movers:
        res.update({
            "ncclAllGather": L.ncclAllGather(fake, fake, count, dt, fake, None),
            "ncclBroadcast": L.ncclBroadcast(fake, fake, count, dt, 0, fake, None),
            "ncclAllToAll": L.ncclAllToAll(fake, fake, count, dt, fake, None),
            "ncclGather": L.ncclGather(fake, fake, count, dt, 0, fake, None),
            "ncclScatter": L.ncclScatter(fake, fake, count, dt, 0, fake, None),
            "ncclSend": L.ncclSend(fake, count, dt, 0, fake, None),
            "ncclRecv": L.ncclRecv(fake, count, dt, 0, fake, None),
        })
    return res


def test_argument_checks_keep_their_order(nccl_lib):
    import mini_nccl as M
    L = nccl_lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced on these paths
    for dt in (10, 11):
        # count == 0 comes before the datatype and the op, as for every datatype
        res = _calls(L, fake, 0, dt, M.ncclSum)
        assert len(res) == 11 and set(res.values()) == {M.ncclSuccess}, res
        # fp8 with ncclAvg (and a negative op): ncclInternalError, before the communicator is read
        for bad_op in (M.ncclAvg, -1):
            res = _calls(L, fake, 4, dt, bad_op, movers=False)
            assert res == {k: M.ncclInternalError for k in FOLDING}, res
        # NULL buffers still win over everything
        assert L.ncclAllReduce(None, fake, 4, dt, M.ncclSum, fake, None) == M.ncclInvalidArgument
        assert L.mncclLocalReduce(fake, None, fake, 4, dt, M.ncclSum, None) == M.ncclInvalidArgument
        # mncclLocalReduce has no communicator: no user ops
        assert L.mncclLocalReduce(fake, fake, fake, 4, dt, M.MNCCL_FIRST_USER_OP, None) == M.ncclInternalError
    # the values next to the new ones are still unsupported, in every call
    for dt in (12, 255):
        res = _calls(L, fake, 4, dt, M.ncclSum)
        assert len(res) == 11 and set(res.values()) == {M.ncclInternalError}, (dt, res)
        arr = (ctypes.c_size_t * 2)(4, 4)
        assert L.ncclAllToAllv(fake, arr, arr, fake, arr, arr, dt, fake, None) == M.ncclInternalError
    # ncclRedOpCreatePreMulSum: NULL arguments first, then the datatype
    op = ctypes.c_int(-1)
    one = ctypes.c_uint8(0x38)
    sc = ctypes.cast(ctypes.byref(one), ctypes.c_void_p)
    host = M.ncclScalarHostImmediate
    for dt in (10, 11):
        assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), sc, dt, host, None) == M.ncclInvalidArgument
        assert L.ncclRedOpCreatePreMulSum(None, sc, dt, host, fake) == M.ncclInvalidArgument
        assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), None, dt, host, fake) == M.ncclInvalidArgument
    for dt in (12, 255):
        assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), None, dt, host, fake) == M.ncclInvalidArgument
        assert L.ncclRedOpCreatePreMulSum(ctypes.byref(op), sc, dt, host, fake) == M.ncclInternalError
    assert op.value == -1  # nothing was written


# ---------------------------------------------------------------- the binding
def test_scalar_bytes():
    import mini_nccl as M
    e4, e5 = M.ncclFloat8e4m3, M.ncclFloat8e5m2
    # an integer is the 8 bits themselves
    assert M.scalar_bytes(0x34, e4).raw[:1] == b"\x34" and M.scalar_bytes(np.uint8(0xC1), e5).raw[:1] == b"\xc1"
    assert M.scalar_bytes(0x34, e4).raw[1:] == bytes(7)
    # a float is rounded by the library's rule: every grid value, midpoint and neighbour, saturation included
    for fmt, dt in (("e4m3", e4), ("e5m2", e5)):
        d = F.decode_table(fmt)
        pos = np.sort(d[np.isfinite(d) & ~np.signbit(d)])
        mid = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
        x = _neighbours(np.concatenate([pos, mid, np.float32([464, 480, 61440, 65536, 1e9, 3.0e38])]))
        x = np.concatenate([x, -x])
        want = F.encode(x, fmt)
        got = np.array([M.scalar_bytes(float(v), dt).raw[0] for v in x], np.uint8)
        assert np.array_equal(got, want), fmt
        assert M.scalar_bytes(np.float32(0.3), dt).raw[0] == F.encode(np.float32([0.3]), fmt)[0]
    assert M.scalar_bytes(1e9, e4).raw[0] == 0x7E and M.scalar_bytes(-1e9, e5).raw[0] == 0xFB
    assert M.scalar_bytes(float("inf"), e5).raw[0] == 0x7C and M.scalar_bytes(float("-inf"), e5).raw[0] == 0xFC
    assert F.is_nan(np.uint8([M.scalar_bytes(float("nan"), e4).raw[0]]), "e4m3").all()
    assert F.is_nan(np.uint8([M.scalar_bytes(float("nan"), e5).raw[0]]), "e5m2").all()
    assert M.scalar_bytes(-0.0, e4).raw[0] == 0x80


# ---------------------------------------------------------------- the kernels as built
EXISTING = (r"(ring|read|oneshot)_kernel|scatter_fold|root_fold|gather_push|root_relay|exchange_push|collect_push|deal_push|"
            r"varblock_push|scaled_(ring|read|scatter|root)|scale_kernel|read_grid_kernel|p2p_kernel|p2p_window_group|local_reduce")


def _built():
    import test_kernel_resources as R
    if not (os.path.exists(R.LIB) and os.path.exists(R.READELF) and os.path.exists(R.OBJDUMP)):
        pytest.skip("library not built / no llvm tools")
    return R


def test_new_kernels_budget_count_and_names(tmp_path):
    R = _built()
    ks = R._kernels(tmp_path)
    new = {k: v for k, v in ks.items() if re.search(r"fp8_|byte_", k)}
    fam = lambda pat: sorted(k for k in new if re.search(pat, k))
    # 2 formats x (4 built-in ops + kPreMulSum) x (vector, element) for the four persistent folds
    for name in ("fp8_ring", "fp8_read", "fp8_scatter", "fp8_root"):
        assert len(fam(name + "I")) == 2 * 5 * 2, (name, fam(name + "I"))
    assert len(fam("fp8_oneshotI")) == 2 * 4 * 2            # no one-shot form of kPreMulSum
    # the grid form: the rule's (G, V) pairs only -- (1, 1), (2, 1), (4, 1), (4, 2), (7, 2) -- x 2 formats x 5 ops
    assert len(fam("fp8_gridI")) == 2 * 5 * 5
    assert len(fam("fp8_scaleI")) == 2
    for name in ("fp8_local_vecI", "fp8_local_gsI", "fp8_local_elemI"):
        assert len(fam(name)) == 2 * 4, name                  # the four built-in ops
    # element size 1 x (vector, element) for the five copy kernels; ncclAllToAllv picks its path at run time
    for name in ("byte_gather", "byte_relay", "byte_exchange", "byte_collect", "byte_deal"):
        assert len(fam(name)) == 2, name
    assert len(fam("byte_varblock")) == 1
    assert len(new) == 4 * 20 + 16 + 50 + 2 + 3 * 8 + 5 * 2 + 1 == 183, sorted(new)
    # none of the names (type names included) is seen by a filter that counts an existing family
    assert not [k for k in new if re.search(EXISTING, k)]
    # the budget every persistent kernel has: two waves per SIMD, no scratch
    over = {k: v for k, v in new.items() if v["vgpr_count"] + v["agpr_count"] > 256}
    assert not over, f"fp8 / byte kernels above 256 registers: {over}"
    spill = {k: v for k, v in new.items() if v["private_segment_fixed_size"] != 0}
    assert not spill, f"fp8 / byte kernels using scratch memory: {spill}"


def test_vector_paths_use_the_packed_conversions(tmp_path):
    """The 16-byte paths of the Sum kernels convert two elements per instruction each way: e4m3 with
    v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32, e5m2 with the bf8 pair -- at least what ONE fold of two
    operand vectors needs, 16 conversions in and 8 out."""
    R = _built()
    fns = R._disassembly_by_kernel(tmp_path)
    forms = (r"fp8_local_vec<{T}, 0>\(", r"fp8_read<{T}, 0, true>\(", r"fp8_ring<{T}, 0, true>\(",
             r"fp8_oneshot<{T}, 0, true>\(", r"fp8_grid<{T}, 0, \d, \d>\(")
    seen = 0
    for T, dec, enc, other in (("mnccl::e4m3_t", "v_cvt_pk_f32_fp8", "v_cvt_pk_fp8_f32", "bf8"),
                               ("mnccl::e5m2_t", "v_cvt_pk_f32_bf8", "v_cvt_pk_bf8_f32", "fp8")):
        for pat in forms:
            rx = re.compile(pat.replace("{T}", re.escape(T)))
            names = [k for k in fns if rx.search(k)]
            assert names, f"no kernel matches {rx.pattern}"
            for k in names:
                # (the mnemonic may carry an encoding suffix: _e32, _e64, _sdwa for the high word)
                nd = len(re.findall(r"\s" + dec + r"(_e32|_e64|_sdwa)?\s", fns[k]))
                ne = len(re.findall(r"\s" + enc + r"(_e32|_e64|_sdwa)?\s", fns[k]))
                assert nd >= 16 and ne >= 8, f"{k}: {nd} x {dec}, {ne} x {enc}"
                assert not re.search(r"\sv_cvt_\w*" + other + r"\w*", fns[k]), f"{k} converts the other format"
                seen += 1
    assert seen == 2 * (4 + 5)  # every form, both formats; the grid form's five (G, V) pairs
