"""ctypes binding of libmini_nccl.so -- the host-side mirror of the reference's C ABI.

The reference's callers are C++ programs linking ``libmini_nccl.so``
(``tests/perf_test.cpp``, ``src/main.cpp``); ``apps/`` holds the C++ equivalents.
This module exposes the same six entry points (``include/mini_nccl_api.h``) plus the
extensions of ``include/mini_nccl_ext.h`` to Python for the test suite and
``bench.py``.  Names, argument meaning and return codes are the C ones: every
function returns an ``ncclResult_t`` integer, exactly as the C ABI does.

Device memory and streams are passed as raw integers (device pointers / hipStream_t),
so any allocator works: torch tensors (``t.data_ptr()``, ``torch.cuda.Stream().cuda_stream``)
or the raw HIP runtime (``tests/hip_rt.py``).  There is no CPU fallback: if the
library is missing, :func:`load` raises.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libmini_nccl.so")

# ncclResult_t (include/mini_nccl_api.h; reference include/mini_nccl_api.h:15-24)
ncclSuccess = 0
ncclUnhandledCudaError = 1
ncclSystemError = 2
ncclInternalError = 3
ncclInvalidArgument = 4
ncclInvalidUsage = 5
ncclRemoteError = 6
ncclInProgress = 7

# ncclDataType_t (reference :29-40)
ncclInt8, ncclUint8, ncclInt32, ncclUint32, ncclInt64, ncclUint64 = 0, 1, 2, 3, 4, 5
ncclFloat16, ncclFloat, ncclDouble, ncclBfloat16 = 6, 7, 8, 9
# the OCP fp8 types (include/mini_nccl_ext.h; NCCL's and RCCL's values)
ncclFloat8e4m3, ncclFloat8e5m2 = 10, 11

# ncclRedOp_t (reference :43-49)
ncclSum, ncclProd, ncclMax, ncclMin, ncclAvg = 0, 1, 2, 3, 4

# ncclScalarResidence_t and the first handle of a user-created op (ncclRedOpCreatePreMulSum)
ncclScalarDevice, ncclScalarHostImmediate = 0, 1
MNCCL_FIRST_USER_OP = 5

# ncclCommSplit: the color of a rank that joins no new communicator
NCCL_SPLIT_NOCOLOR = -1

# mncclAlgo_t (mncclAlgoDirect = 1 was removed in mncclVersion 400)
ALGO_AUTO, ALGO_RING, ALGO_READ, ALGO_ONESHOT, ALGO_READ_GRID = -1, 0, 2, 3, 4

DTYPE_SIZE = {ncclInt32: 4, ncclFloat16: 2, ncclFloat: 4, ncclDouble: 8, ncclBfloat16: 2,
              ncclFloat8e4m3: 1, ncclFloat8e5m2: 1}


class CommInfo(ctypes.Structure):
    _fields_ = [
        ("rank", ctypes.c_int), ("nranks", ctypes.c_int), ("device", ctypes.c_int),
        ("slice_bytes", ctypes.c_size_t), ("window", ctypes.c_int), ("signal_batch", ctypes.c_int),
        ("channels", ctypes.c_int), ("slots", ctypes.c_int), ("threads", ctypes.c_int),
        ("algo", ctypes.c_int), ("blocking", ctypes.c_int), ("sys_fence", ctypes.c_int),
        ("timeout_s", ctypes.c_double), ("scratch_bytes", ctypes.c_size_t), ("tune_ms", ctypes.c_double * 2),
        ("pipelines", ctypes.c_int), ("ranks_on_device", ctypes.c_int), ("slot_bytes", ctypes.c_size_t),
        ("last_algo", ctypes.c_int), ("peer_mappings", ctypes.c_size_t), ("scratch_algo", ctypes.c_int),
        ("calib_choice", ctypes.c_int), ("calib_ms", ctypes.c_double * 2),
        # since mncclVersion 300
        ("ipc_open_failures", ctypes.c_ulonglong), ("read_map_failures", ctypes.c_ulonglong),
        ("read_rounds", ctypes.c_ulonglong), ("closed_freed", ctypes.c_ulonglong), ("live_exports", ctypes.c_size_t),
        # since mncclVersion 400
        ("cap_refusals", ctypes.c_ulonglong), ("liveness_queries", ctypes.c_ulonglong), ("read_push", ctypes.c_int),
        # since mncclVersion 500
        ("auto_read", ctypes.c_int), ("peer_link", ctypes.c_int * 16), ("peer_hops", ctypes.c_int * 16),
        ("auto_reason", ctypes.c_char * 160), ("read_grid_calls", ctypes.c_ulonglong),
        ("window_calls", ctypes.c_ulonglong), ("windows", ctypes.c_int), ("auto_grid", ctypes.c_int),
        # since mncclVersion 501
        ("retired_imports", ctypes.c_int),
        # since mncclVersion 600
        ("retired_bytes", ctypes.c_ulonglong), ("retired_budget", ctypes.c_ulonglong),
        ("budget_refusals", ctypes.c_ulonglong), ("window_fast", ctypes.c_int),
        ("run_pipelines", ctypes.c_int),
        # still 600: point to point on registered windows
        ("p2p_direct_recvs", ctypes.c_ulonglong), ("p2p_direct_sends", ctypes.c_ulonglong),
    ]


# every entry point of include/mini_nccl_api.h and include/mini_nccl_ext.h: (restype, argtypes)
_VP, _SZ, _I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
SIGNATURES = {
    "ncclGetErrorString": (ctypes.c_char_p, [_I]),
    "ncclCommInitRank": (_I, [ctypes.POINTER(_VP), _I, _I, ctypes.c_char_p]),
    "ncclCommDestroy": (_I, [_VP]),
    "ncclCommUserRank": (_I, [_VP, ctypes.POINTER(_I)]),
    "ncclCommCount": (_I, [_VP, ctypes.POINTER(_I)]),
    "ncclAllReduce": (_I, [_VP, _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclReduceScatter": (_I, [_VP, _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclAllGather": (_I, [_VP, _VP, _SZ, _I, _VP, _VP]),
    "ncclBroadcast": (_I, [_VP, _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclReduce": (_I, [_VP, _VP, _SZ, _I, _I, _I, _VP, _VP]),
    "ncclAllToAll": (_I, [_VP, _VP, _SZ, _I, _VP, _VP]),
    "ncclAllToAllv": (_I, [_VP, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ), _VP, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ),
                           _I, _VP, _VP]),
    "mncclAllGatherv": (_I, [_VP, _SZ, _VP, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ), _I, _VP, _VP]),
    "mncclReduceScatterv": (_I, [_VP, ctypes.POINTER(_SZ), ctypes.POINTER(_SZ), _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclGather": (_I, [_VP, _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclScatter": (_I, [_VP, _VP, _SZ, _I, _I, _VP, _VP]),
    "ncclSend": (_I, [_VP, _SZ, _I, _I, _VP, _VP]),
    "ncclRecv": (_I, [_VP, _SZ, _I, _I, _VP, _VP]),
    "ncclGroupStart": (_I, []),
    "ncclGroupEnd": (_I, []),
    "ncclRedOpCreatePreMulSum": (_I, [ctypes.POINTER(_I), _VP, _I, _I, _VP]),
    "ncclRedOpDestroy": (_I, [_I, _VP]),
    "ncclCommSplit": (_I, [_VP, _I, _I, ctypes.POINTER(_VP), _VP]),
    "mncclLocalReduce": (_I, [_VP, _VP, _VP, _SZ, _I, _I, _VP]),
    "mncclDataTypeSize": (_I, [_I, ctypes.POINTER(_SZ)]),
    "mncclCommGetAsyncError": (_I, [_VP, ctypes.POINTER(_I)]),
    "mncclCommGetInfo": (_I, [_VP, ctypes.POINTER(CommInfo)]),
    "mncclCommGetInfoV": (_I, [_VP, _VP, _SZ]),
    "mncclCommSetAlgo": (_I, [_VP, _I]),
    "mncclCommLinkProbe": (_I, [_VP, _I, _SZ, _I, ctypes.POINTER(ctypes.c_double)]),
    "mncclCommRegister": (_I, [_VP, _VP, _SZ, ctypes.POINTER(_VP)]),
    "mncclCommDeregister": (_I, [_VP, _VP]),
    "mncclVersion": (_I, []),
}

_lib = None


def load(path=None):
    """Load libmini_nccl.so (raises OSError if it is missing: no fallback)."""
    global _lib
    if _lib is None or path is not None:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise OSError(f"{p} not built: run `make -C mini-nccl_amd` (or __graft_entry__.build())")
        lib = ctypes.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def get_error_string(result):
    return load().ncclGetErrorString(int(result)).decode()


class NcclError(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__(f"{what}: {get_error_string(code)} ({code})")
        self.code = code


def check(code, what="mini-nccl"):
    if code != ncclSuccess:
        raise NcclError(code, what)
    return code


def _fp8_encode(value, ebits, mbits, bias, has_inf):
    """One float as an OCP fp8 byte by the library's rule (mini_nccl_ext.h): nearest even onto the
    finite grid, subnormals included; a finite value beyond the largest finite one saturates to it;
    NaN stays NaN, +-inf stays +-inf where the format has it (e5m2) and is NaN where it has not."""
    import math
    from fractions import Fraction
    sign = 0x80 if math.copysign(1.0, value) < 0 else 0
    nan = 0x7F  # (a NaN of either format)
    if math.isnan(value):
        return sign | nan
    top = (1 << ebits) - 1                      # the largest exponent field
    max_e = top - 1 if has_inf else top         # ... that holds finite values
    max_m = (1 << mbits) - 1 if has_inf else (1 << mbits) - 2  # e4m3fn: the all-ones code is NaN
    max_code = (max_e << mbits) | max_m
    if math.isinf(value):
        return sign | ((top << mbits) if has_inf else nan)
    a = Fraction(abs(value))
    if a == 0:
        return sign
    # the grid's step at a: 2^(e - bias - mbits) with e the biased exponent, at least 1 (subnormals)
    e = max(1, min(max_e, (a.numerator.bit_length() - a.denominator.bit_length()) + bias + 1))
    while e > 1 and a < Fraction(2) ** (e - bias):
        e -= 1
    while e < max_e and a >= Fraction(2) ** (e + 1 - bias):
        e += 1
    q = a / Fraction(2) ** (e - bias - mbits)    # in units of the step: [2^mbits, 2^(mbits+1)) if normal
    k = q.numerator // q.denominator
    r = q - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k & 1):
        k += 1
    code = ((e - 1) << mbits) + k                # (a carry out of the mantissa moves into the exponent)
    return sign | min(code, max_code)


def scalar_bytes(scalar, dtype):
    """One value of `dtype` as a ctypes buffer (what ncclRedOpCreatePreMulSum reads through its
    `scalar` pointer).  A number is converted to the datatype, rounded to nearest even.  For
    ncclBfloat16 and the fp8 types an integer (a Python int or a numpy integer such as numpy.uint16)
    is taken as the 16 / 8 bits themselves, since numpy has no such scalar to pass; an fp8 float is
    rounded by the library's own rule (saturating)."""
    import numbers
    import struct
    if dtype == ncclFloat:
        raw = struct.pack("<f", float(scalar))
    elif dtype == ncclDouble:
        raw = struct.pack("<d", float(scalar))
    elif dtype == ncclInt32:
        raw = struct.pack("<i", int(scalar))
    elif dtype == ncclFloat16:
        raw = struct.pack("<e", float(scalar))
    elif dtype == ncclBfloat16:
        if isinstance(scalar, numbers.Integral):
            raw = struct.pack("<H", int(scalar))
        else:
            u = struct.unpack("<I", struct.pack("<f", float(scalar)))[0]
            raw = struct.pack("<H", ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF)
    elif dtype in (ncclFloat8e4m3, ncclFloat8e5m2):
        if isinstance(scalar, numbers.Integral):
            raw = struct.pack("<B", int(scalar) & 0xFF)
        elif dtype == ncclFloat8e4m3:
            raw = struct.pack("<B", _fp8_encode(float(scalar), 4, 3, 7, False))
        else:
            raw = struct.pack("<B", _fp8_encode(float(scalar), 5, 2, 15, True))
    else:
        raw = bytes(8)  # an unsupported datatype: the library refuses it before it reads the scalar
    return ctypes.create_string_buffer(raw, 8)


class Comm:
    """Thin RAII wrapper over ncclComm_t (the calls themselves are the C functions)."""

    def __init__(self, nranks, rank, ip="127.0.0.1"):
        lib = load()
        self.handle = ctypes.c_void_p()
        check(lib.ncclCommInitRank(ctypes.byref(self.handle), nranks, rank, ip.encode() if ip else None),
              "ncclCommInitRank")

    @classmethod
    def _adopt(cls, handle):
        c = cls.__new__(cls)
        c.handle = handle
        return c

    def split_rc(self, color, key=0):
        """ncclCommSplit's result code (does not raise) and the new Comm, or None where the library
        returned no communicator (NCCL_SPLIT_NOCOLOR, or a failure)."""
        h = ctypes.c_void_p()
        rc = load().ncclCommSplit(self.handle, int(color), int(key), ctypes.byref(h), None)
        return rc, (Comm._adopt(h) if rc == ncclSuccess and h else None)

    def split(self, color, key=0):
        """ncclCommSplit (collective over this communicator's ranks): the ranks passing the same
        color >= 0 form a new communicator, ordered by key (ties: by the rank here).  Returns the new
        Comm, or None for NCCL_SPLIT_NOCOLOR.  The child is independent of this communicator and is
        destroyed on its own."""
        rc, child = self.split_rc(color, key)
        check(rc, "ncclCommSplit")
        return child

    def all_reduce(self, send_ptr, recv_ptr, count, dtype=ncclFloat, op=ncclSum, stream=0):
        """Returns the ncclResult_t (does not raise) -- the reference's calling convention."""
        return load().ncclAllReduce(send_ptr, recv_ptr, count, dtype, op, self.handle, stream)

    def reduce_scatter(self, send_ptr, recv_ptr, recvcount, dtype=ncclFloat, op=ncclSum, stream=0):
        """ncclReduceScatter: send holds nranks * recvcount elements, recv gets chunk `rank` of
        their all-reduce (the same bits).  Returns the ncclResult_t."""
        return load().ncclReduceScatter(send_ptr, recv_ptr, recvcount, dtype, op, self.handle, stream)

    def all_gather(self, send_ptr, recv_ptr, sendcount, dtype=ncclFloat, stream=0):
        """ncclAllGather: recv holds nranks * sendcount elements, rank q's send at
        [q * sendcount, (q + 1) * sendcount).  Returns the ncclResult_t."""
        return load().ncclAllGather(send_ptr, recv_ptr, sendcount, dtype, self.handle, stream)

    def broadcast(self, send_ptr, recv_ptr, count, dtype=ncclFloat, root=0, stream=0):
        """ncclBroadcast: every rank's recv gets the root's `count` elements of send (send is read on
        the root only: elsewhere it may be 0 / None)."""
        return load().ncclBroadcast(send_ptr, recv_ptr, count, dtype, root, self.handle, stream)

    def reduce(self, send_ptr, recv_ptr, count, dtype=ncclFloat, op=ncclSum, root=0, stream=0):
        """ncclReduce: the root's recv gets the reduction of every rank's `count` elements of send
        (recv is written on the root only: elsewhere it may be 0 / None and is never touched)."""
        return load().ncclReduce(send_ptr, recv_ptr, count, dtype, op, root, self.handle, stream)

    def all_to_all(self, send_ptr, recv_ptr, count, dtype=ncclFloat, stream=0):
        """ncclAllToAll: send and recv each hold nranks * count elements; block q of this rank's send
        becomes block `rank` of rank q's recv (no in-place form).  Returns the ncclResult_t."""
        return load().ncclAllToAll(send_ptr, recv_ptr, count, dtype, self.handle, stream)

    def all_to_all_v(self, send_ptr, sendcounts, sdispls, recv_ptr, recvcounts, rdispls, dtype=ncclFloat, stream=0):
        """ncclAllToAllv: elements [sdispls[q], sdispls[q] + sendcounts[q]) of this rank's send become
        elements [rdispls[r], rdispls[r] + recvcounts[r]) of rank q's recv.  The four arguments are
        Python sequences of nranks element counts / displacements (read before the call returns);
        a rank whose counts are all zero may pass 0 / None for its buffers.  Returns the ncclResult_t."""
        arrays = [(ctypes.c_size_t * len(a))(*[int(x) for x in a]) for a in (sendcounts, sdispls, recvcounts, rdispls)]
        return load().ncclAllToAllv(send_ptr, arrays[0], arrays[1], recv_ptr, arrays[2], arrays[3], dtype, self.handle,
                                    stream)

    def all_gather_v(self, send_ptr, sendcount, recv_ptr, recvcounts, rdispls, dtype=ncclFloat, stream=0):
        """mncclAllGatherv: rank q's `sendcount` elements of send end up at elements [rdispls[q],
        rdispls[q] + recvcounts[q]) of every rank's recv.  recvcounts / rdispls are Python sequences of
        nranks entries, the same on every rank (read before the call returns); sendcount must be
        recvcounts[rank]; a rank whose block is empty may pass 0 / None for send.  In place: send is
        recv + rdispls[rank] elements.  Returns the ncclResult_t."""
        arrays = [(ctypes.c_size_t * len(a))(*[int(x) for x in a]) for a in (recvcounts, rdispls)]
        return load().mncclAllGatherv(send_ptr, sendcount, recv_ptr, arrays[0], arrays[1], dtype, self.handle, stream)

    def reduce_scatter_v(self, send_ptr, sendcounts, sdispls, recv_ptr, recvcount, dtype=ncclFloat, op=ncclSum,
                         stream=0):
        """mncclReduceScatterv: recv gets the reduction over all ranks of elements [sdispls[rank],
        sdispls[rank] + sendcounts[rank]) of their send, in ncclReduceScatter's association.
        sendcounts / sdispls are Python sequences of nranks entries, the same on every rank;
        recvcount must be sendcounts[rank]; a rank whose block is empty may pass 0 / None for recv.  In
        place: recv is send + sdispls[rank] elements.  Returns the ncclResult_t."""
        arrays = [(ctypes.c_size_t * len(a))(*[int(x) for x in a]) for a in (sendcounts, sdispls)]
        return load().mncclReduceScatterv(send_ptr, arrays[0], arrays[1], recv_ptr, recvcount, dtype, op, self.handle,
                                          stream)

    def gather(self, send_ptr, recv_ptr, sendcount, dtype=ncclFloat, root=0, stream=0):
        """ncclGather: the root's recv holds nranks * sendcount elements, rank q's send at
        [q * sendcount, (q + 1) * sendcount) (recv is written on the root only: elsewhere it may be
        0 / None and is never touched).  Returns the ncclResult_t."""
        return load().ncclGather(send_ptr, recv_ptr, sendcount, dtype, root, self.handle, stream)

    def scatter(self, send_ptr, recv_ptr, recvcount, dtype=ncclFloat, root=0, stream=0):
        """ncclScatter: the root's send holds nranks * recvcount elements, this rank's recv gets block
        `rank` of it (send is read on the root only: elsewhere it may be 0 / None).  Returns the
        ncclResult_t."""
        return load().ncclScatter(send_ptr, recv_ptr, recvcount, dtype, root, self.handle, stream)

    def send(self, send_ptr, count, dtype=ncclFloat, peer=0, stream=0):
        """ncclSend: `count` elements to rank `peer`; inside a group (group_start / group) it is only
        recorded.  Returns the ncclResult_t."""
        return load().ncclSend(send_ptr, count, dtype, peer, self.handle, stream)

    def recv(self, recv_ptr, count, dtype=ncclFloat, peer=0, stream=0):
        """ncclRecv: `count` elements from rank `peer`, matching its sends to this rank in call order.
        Returns the ncclResult_t."""
        return load().ncclRecv(recv_ptr, count, dtype, peer, self.handle, stream)

    def redop_premul_sum_rc(self, scalar, dtype=ncclFloat, residence=ncclScalarHostImmediate):
        """ncclRedOpCreatePreMulSum's result code (does not raise) and the handle.  `scalar`: as
        scalar_bytes takes it (a number; for ncclBfloat16 an integer is the 16 bits)."""
        buf = scalar_bytes(scalar, dtype)
        op = ctypes.c_int(-1)
        rc = load().ncclRedOpCreatePreMulSum(ctypes.byref(op), ctypes.cast(buf, ctypes.c_void_p), dtype, residence,
                                             self.handle)
        return rc, op.value

    def redop_premul_sum(self, scalar, dtype=ncclFloat):
        """ncclRedOpCreatePreMulSum: an op of this communicator that all_reduce, reduce_scatter and
        reduce accept in place of ncclSum; every input is multiplied by `scalar` (one value of
        `dtype`, the same on every rank) on its way into the sum.  Returns the handle."""
        rc, op = self.redop_premul_sum_rc(scalar, dtype)
        check(rc, "ncclRedOpCreatePreMulSum")
        return op

    def redop_destroy(self, op):
        """ncclRedOpDestroy: returns the ncclResult_t.  Allowed as soon as the last call using the op
        has been issued."""
        return load().ncclRedOpDestroy(int(op), self.handle)

    def rank(self):
        r = ctypes.c_int()
        check(load().ncclCommUserRank(self.handle, ctypes.byref(r)))
        return r.value

    def count(self):
        c = ctypes.c_int()
        check(load().ncclCommCount(self.handle, ctypes.byref(c)))
        return c.value

    def info(self):
        i = CommInfo()
        check(load().mncclCommGetInfoV(self.handle, ctypes.byref(i), ctypes.sizeof(i)))
        d = {f: getattr(i, f) for f, _ in CommInfo._fields_}
        d["tune_ms"] = list(d["tune_ms"])
        d["calib_ms"] = list(d["calib_ms"])
        n = d["nranks"]
        d["peer_link"] = list(d["peer_link"])[:n]
        d["peer_hops"] = list(d["peer_hops"])[:n]
        d["auto_reason"] = d["auto_reason"].decode(errors="replace")
        return d

    PROBE_FORMS = {"sys": 0, "nt": 1, "plain": 2}

    def link_probe(self, all_peers=False, nbytes=0, iters=10, form="sys", pull=False, user=False):
        """GB/s per destination link (collective: every rank must call it).  form: the remote
        accesses' cache policy ("sys" = the hot path's sc0 sc1, "nt", "plain"); pull: load
        from the peers over the link instead of storing into them; user: the peers' ordinary
        device memory (what the read schedule loads from) instead of their uncached scratch."""
        g = ctypes.c_double()
        mode = int(bool(all_peers)) | (self.PROBE_FORMS[form] << 1) | (8 if pull else 0) | (16 if user else 0)
        check(load().mncclCommLinkProbe(self.handle, mode, nbytes, iters, ctypes.byref(g)), "mncclCommLinkProbe")
        return g.value

    def register(self, ptr, nbytes):
        """mncclCommRegister (collective): returns the window handle."""
        h = ctypes.c_void_p()
        check(load().mncclCommRegister(self.handle, ptr, nbytes, ctypes.byref(h)), "mncclCommRegister")
        return h

    def register_rc(self, ptr, nbytes):
        """mncclCommRegister's result code (does not raise) and the handle."""
        h = ctypes.c_void_p()
        return load().mncclCommRegister(self.handle, ptr, nbytes, ctypes.byref(h)), h

    def deregister(self, h):
        return check(load().mncclCommDeregister(self.handle, h), "mncclCommDeregister")

    def set_algo(self, algo):
        return check(load().mncclCommSetAlgo(self.handle, algo))

    def async_error(self):
        e = ctypes.c_int()
        check(load().mncclCommGetAsyncError(self.handle, ctypes.byref(e)))
        return e.value

    def destroy(self):
        if self.handle:
            code = load().ncclCommDestroy(self.handle)
            self.handle = ctypes.c_void_p()
            return code
        return ncclSuccess


def group_start():
    """ncclGroupStart: open (or nest) this thread's group.  Returns the ncclResult_t."""
    return load().ncclGroupStart()


def group_end():
    """ncclGroupEnd: the outermost one launches every recorded send / recv as one kernel launch.
    Returns the ncclResult_t (the group's first error, if an operation failed)."""
    return load().ncclGroupEnd()


class group:
    """``with mini_nccl.group() as g: comm.send(...); comm.recv(...)`` -- ncclGroupStart on entry,
    ncclGroupEnd on exit; ``g.rc`` is ncclGroupEnd's ncclResult_t (nothing raises)."""

    def __init__(self):
        self.rc = None

    def __enter__(self):
        group_start()
        return self

    def __exit__(self, *exc):
        self.rc = group_end()
        return False


def local_reduce(out_ptr, local_ptr, incoming_ptr, count, dtype=ncclFloat, op=ncclSum, stream=0):
    """out[i] = op(local[i], incoming[i]) on the GPU (the scatter-reduce element-wise kernel)."""
    return load().mncclLocalReduce(out_ptr, local_ptr, incoming_ptr, count, dtype, op, stream)


def data_type_size(dtype):
    """mncclDataTypeSize: (ncclResult_t, element size in bytes or None)."""
    n = ctypes.c_size_t(0)
    rc = load().mncclDataTypeSize(int(dtype), ctypes.byref(n))
    return rc, (n.value if rc == ncclSuccess else None)
