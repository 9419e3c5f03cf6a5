// kernels.hip -- the hot path, hand-written for CDNA4 (gfx950).
//
//  ring_kernel    persistent ring all-reduce (reference mini_nccl.cu:56-217 re-designed):
//                 one WAVE per pipeline (channel), each an independent slice pipeline; the
//                 reference's per-slice launches of wait_kernel (:22-30),
//                 elementwise_reduce_kernel (:43-47), the IPC memcpy (:131,:174) and
//                 set_flag_kernel (:32-36) become one launch per call in which every
//                 pipeline moves its slices through a `slots`-deep FIFO in the next
//                 rank's scratch with epoch-free monotone flags and explicit credits.
//                 Default geometry: 256 one-wave workgroups = one pipeline per CU.
//  read_kernel    the default: same association order, no scratch -- each rank loads its
//                 peers' send buffers over the links and pushes its results into their recv
//                 buffers (mapped by Comm per allocation).
//  scatter_fold / gather_push   the read schedule's two halves as collectives of their own
//                 (ncclReduceScatter / ncclAllGather): read_kernel's fold without its pushes, and
//                 its pushes without a fold; the same protocol, so calls of any kind follow each
//                 other on one communicator.  Their fallback is ring_kernel with the op table of
//                 one half (schedule.h coll_op).
//  root_fold / root_relay   the rooted collectives (ncclReduce / ncclBroadcast) on the same
//                 protocol: every rank folds, or copies out of the root's send, chunk `rank` only,
//                 so no link carries the whole buffer.  Their fallback is ring_kernel too.
//                 root_relay and gather_push run one loop (copy_push_slice): load a slice once,
//                 store it into this rank's recv and push it into the other ranks'.
//  exchange_push  the all-to-all (ncclAllToAll) on the same protocol: every rank pushes block q of
//                 its own send into rank q's recv, so every block crosses one link once.  Its
//                 fallback is ring_kernel with a table of hops (schedule.h coll_op).
//  collect_push / deal_push   gather and scatter (ncclGather / ncclScatter) on the same protocol:
//                 column `root` and row `root` of the all-to-all -- every rank pushes its one block
//                 into the root's recv; the root pushes block q of its send into rank q's recv.
//                 Their fallback is ring_kernel with a chain's table (schedule.h coll_op).
//  varblock_push  the variable all-to-all (ncclAllToAllv) on the same protocol: exchange_push with a
//                 length and two offsets per destination, the slices cut for the largest block of
//                 the whole matrix.  Its fallback is the ring's all-to-all on padded blocks.
//  vhalf_fold / vhalf_push   the halves with per-rank counts (mncclReduceScatterv / mncclAllGatherv)
//                 on the same protocol: scatter_fold and gather_push with a per-rank base and
//                 length, the slices cut for the largest block.  Their fallback is the ring's
//                 halves on padded blocks.
//  p2p_kernel     point to point (ncclSend / ncclRecv, one launch per group): a send is the sender's
//                 half of one ring hop to an arbitrary peer, a recv the receiver's half, on the
//                 ring's scratch, flags and counters; every directed pair of the group on waves of
//                 its own, one per pipeline, so no wave ever waits for two peers.
//  p2p_window_group   the same groups on a communicator with registered windows: the receiver posts a
//                 destination per message from the device, and the sender pushes straight into a recv
//                 that lies in a window (one pass over the bytes), else through the scratch.
//  read_start / read_grid / read_done   the read schedule's push form as three launches (the
//                 runtime form mncclAlgoReadGrid, for large calls): a grid of one-batch workgroups
//                 between a one-wave START and a one-wave DONE.
//  oneshot_kernel small calls the read schedule cannot take (host buffers): one hand-off -- every
//                 rank stores its pieces into every peer's scratch and folds the result itself,
//                 same association order.
//  local_reduce   the element-wise op alone: out = op(local, incoming), 16 B per lane.
//  fp8_* / byte_*  the same bodies for the one-byte datatypes (ncclFloat8e4m3 / ncclFloat8e5m2, OCP): the
//                 kernels that fold under fp8_* names (element ops over gfx950's packed fp8 conversions,
//                 saturating), the kernels that only copy under byte_* names (element size 1).
//
// Memory-ordering protocol (cross-process, cross-device over xGMI):
//  * everything another rank writes in the ring lives in THIS rank's scratch / mailbox,
//    allocated hipDeviceMallocUncached: no cache of any agent keeps a copy of those lines;
//  * payload stores to a peer's slot are sc0 sc1 16-byte buffer stores (the instruction a
//    system-scope atomic store is; write-through, nothing left dirty in an L2); the wave
//    drains (s_waitcnt vmcnt(0) in asm, so the compiler cannot drop it) and lane 0 stores
//    the READY word with a system-scope atomic store;
//  * the consumer polls its own READY word with system-scope relaxed loads from lane 0
//    (s_sleep between polls) and reads the slot with sc0 sc1 loads (system-scope atomic
//    loads: they bypass L1/L2 whatever the mapping), so neither a release fence before
//    the flag nor an acquire fence after the poll is needed (cdna_hip_programming.md
//    Guideline 16's sc1 form); MINI_NCCL_SYS_FENCE=1 adds both (system scope);
//  * after the drain that follows the last load of a slot, lane 0 returns a CREDIT to
//    the sender; the sender reuses a slot only after the credit for the message that
//    last used it (seq - slots) arrived.
//  * flags are monotone 64-bit sequence numbers per (peer, pipeline) that continue across
//    calls (kept in device memory and advanced by the kernel itself, so graph replays stay
//    consistent); nothing is reset per call and stale flags cannot satisfy a wait.
//  * every spin is bounded (MINI_NCCL_TIMEOUT_MS via s_memrealtime) and also exits on
//    the host abort word or a peer's ABORT; the kernel always terminates.
//  * read_kernel loads the peers' send buffers with the same sc0 sc1 loads, after their START
//    (their send is in memory: every kernel before the call ended and wrote its data back),
//    and pushes its result slices into their recv with sc0 sc1 stores, drained before DONE.
//    Why the owner's later kernels then read the pushed bytes and not stale lines its L2 kept
//    of recv from before the call: a write that reaches memory from a CU under another L2
//    invalidates this L2's copy of the line, and an sc0 sc1 store is acknowledged only once it
//    has reached memory (measured across the eight L2s of one MI355X with no kernel boundary:
//    tools/probe_xcd_coherence.hip, profiles/r4_xcd_coherence.txt; DESIGN.md "Coherence of the
//    pushes").  Plain or non-temporal stores would NOT do: they are acknowledged from the
//    writer's L2 and the owner's stale line survives (same probe).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "schedule.h"

namespace mnccl {

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef uint64_t u64;
typedef __amdgpu_buffer_rsrc_t rsrc_t;

constexpr int kAuxSys = 17;  // sc0 | sc1: system-coherent buffer access

struct bf16_t { uint16_t v; };

// ---------------------------------------------------------------- element ops
// c = op(a = local, b = incoming), reference mini_nccl.cu:38-41
template <typename T, int OPC> struct Op;
template <typename T> struct Op<T, kSum> { __device__ static T f(T a, T b) { return a + b; } };
template <typename T> struct Op<T, kProd> { __device__ static T f(T a, T b) { return a * b; } };
template <typename T> struct Op<T, kMax> { __device__ static T f(T a, T b) { return (a > b) ? a : b; } };
template <typename T> struct Op<T, kMin> { __device__ static T f(T a, T b) { return (a < b) ? a : b; } };
// int32 +,*: two's-complement wrap (no signed-overflow UB)
template <> struct Op<int32_t, kSum> {
  __device__ static int32_t f(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
};
template <> struct Op<int32_t, kProd> {
  __device__ static int32_t f(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
};
// bf16: widen (exact), op in f32, round to nearest even (correctly rounded: 24 >= 2*8+2) with
// the hardware's v_cvt_pk_bf16_f32 (gfx950; the compiler pairs two elements per instruction);
// NaN stays NaN (its payload is the hardware's, as IEEE leaves it to the implementation)
__device__ __forceinline__ float bf2f(bf16_t x) { return __uint_as_float((uint32_t)x.v << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  bf16_t r;
  r.v = __builtin_bit_cast(uint16_t, (__bf16)f);
  return r;
}
template <> struct Op<bf16_t, kSum> { __device__ static bf16_t f(bf16_t a, bf16_t b) { return f2bf(bf2f(a) + bf2f(b)); } };
template <> struct Op<bf16_t, kProd> { __device__ static bf16_t f(bf16_t a, bf16_t b) { return f2bf(bf2f(a) * bf2f(b)); } };
template <> struct Op<bf16_t, kMax> { __device__ static bf16_t f(bf16_t a, bf16_t b) { return (bf2f(a) > bf2f(b)) ? a : b; } };
template <> struct Op<bf16_t, kMin> { __device__ static bf16_t f(bf16_t a, bf16_t b) { return (bf2f(a) < bf2f(b)) ? a : b; } };

// fp8, OCP encodings (ncclFloat8e4m3 = e4m3fn: bias 7, no infinities, NaN 0x7f / 0xff, largest finite
// 448; ncclFloat8e5m2: bias 15, IEEE-like, largest finite 57344) -- bf16's rule one format down: widen
// (exact), ONE f32 operation (the product of two fp8 values is exact in f32), round once to nearest
// even onto the type's finite grid, subnormals included, with gfx950's packed conversions, two elements
// per instruction each way (v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32 and the bf8 pair; the word of the dword
// they read or write is an op_sel bit).  A finite result beyond the largest finite value saturates to
// it and never becomes inf or NaN: fp8_sat clamps every value whose f32 exponent is not all ones ahead
// of the conversion (amd_hip_fp8.h's saturating cast does the same), so the conversion itself never
// sees a finite value out of range; NaN stays a NaN of the type, +-inf stays +-inf for e5m2 (e4m3 has
// no operand that could produce one), the sign of zero is the f32 result's.  Max and Min compare the
// decoded values and return an operand's byte unchanged, with bf16's expression.
struct e4m3_t { uint8_t v; };
struct e5m2_t { uint8_t v; };
typedef float v2f __attribute__((ext_vector_type(2)));

template <typename T> struct IsFp8 : std::false_type {};
template <> struct IsFp8<e4m3_t> : std::true_type {};
template <> struct IsFp8<e5m2_t> : std::true_type {};

// dec2<HI>(w): bytes 2 HI, 2 HI + 1 of w as two floats; enc2<HI>(a, b, old): old with those bytes replaced
template <typename T> struct Fp8;
template <> struct Fp8<e4m3_t> {
  static constexpr float kMax = 448.0f;
  template <bool HI> __device__ static v2f dec2(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI); }
  template <bool HI> __device__ static uint32_t enc2(float a, float b, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, HI);
  }
};
template <> struct Fp8<e5m2_t> {
  static constexpr float kMax = 57344.0f;
  template <bool HI> __device__ static v2f dec2(uint32_t w) { return __builtin_amdgcn_cvt_pk_f32_bf8((int)w, HI); }
  template <bool HI> __device__ static uint32_t enc2(float a, float b, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, (int)old, HI);
  }
};

template <typename T>
__device__ __forceinline__ float fp8_sat(float r) {
  return (__float_as_uint(r) & 0x7f800000u) != 0x7f800000u ? __builtin_amdgcn_fmed3f(r, Fp8<T>::kMax, -Fp8<T>::kMax) : r;
}

// op(a, b) on the two elements in word HI of a and b, written into that word of old
template <typename T, int OPC, bool HI>
__device__ __forceinline__ uint32_t fp8_fold2(uint32_t a, uint32_t b, uint32_t old) {
  const v2f fa = Fp8<T>::template dec2<HI>(a), fb = Fp8<T>::template dec2<HI>(b);
  if constexpr (OPC == kMax || OPC == kMin) {
    const bool t0 = OPC == kMax ? fa.x > fb.x : fa.x < fb.x, t1 = OPC == kMax ? fa.y > fb.y : fa.y < fb.y;
    constexpr uint32_t word = HI ? 0xffff0000u : 0x0000ffffu;
    const uint32_t m = ((t0 ? 0x00ff00ffu : 0u) | (t1 ? 0xff00ff00u : 0u)) & word;  // bytes taken from a
    return (old & ~word) | (a & m) | (b & ~m & word);
  } else {
    const v2f r = OPC == kProd ? fa * fb : fa + fb;
    return Fp8<T>::template enc2<HI>(fp8_sat<T>(r.x), fp8_sat<T>(r.y), old);
  }
}
template <typename T, int OPC>
__device__ __forceinline__ uint32_t fp8_fold4(uint32_t a, uint32_t b) {
  return fp8_fold2<T, OPC, true>(a, b, fp8_fold2<T, OPC, false>(a, b, 0u));
}
// s * x on the two elements in word HI of x (s: one fp8 value in the low byte), one rounding
template <typename T, bool HI>
__device__ __forceinline__ uint32_t fp8_scale2(uint32_t s, uint32_t x, uint32_t old) {
  const float fs = Fp8<T>::template dec2<false>(s & 0xffu).x;
  const v2f r = Fp8<T>::template dec2<HI>(x) * fs;
  return Fp8<T>::template enc2<HI>(fp8_sat<T>(r.x), fp8_sat<T>(r.y), old);
}

#define MNCCL_FP8_OP(T, OPC)                                          \
  template <> struct Op<T, OPC> {                                     \
    __device__ static T f(T a, T b) {                                 \
      T r;                                                            \
      r.v = (uint8_t)fp8_fold2<T, OPC, false>(a.v, b.v, 0u);          \
      return r;                                                       \
    }                                                                 \
  };
MNCCL_FP8_OP(e4m3_t, kSum) MNCCL_FP8_OP(e4m3_t, kProd) MNCCL_FP8_OP(e4m3_t, kMax) MNCCL_FP8_OP(e4m3_t, kMin)
MNCCL_FP8_OP(e5m2_t, kSum) MNCCL_FP8_OP(e5m2_t, kProd) MNCCL_FP8_OP(e5m2_t, kMax) MNCCL_FP8_OP(e5m2_t, kMin)
#undef MNCCL_FP8_OP


// kPreMulSum (ncclRedOpCreatePreMulSum): the sum of inputs that were scaled on their way in.  Every
// rank's input element becomes y = round_T(s * x) where it enters a fold (prescale below) -- ONE
// correctly rounded multiplication in T's arithmetic (f16: the f16 product; bf16: the f32 product,
// exact, rounded to nearest even; int32: two's-complement wrap) -- and the y are then summed exactly
// as kSum sums them, packed adds included.  s is the call's scalar, the same on every rank, by
// value in CollParams::scale (wave-uniform: it stays in SGPRs).  The product and the sum stay two
// roundings: the ring scales a chunk in one message body and adds to it in another, so a fold that
// fused them would disagree with it.  hipcc contracts a * b + c by default; the pragma keeps the
// multiplication out of that, here only -- every other kernel compiles as it did.
template <typename T> struct Op<T, kPreMulSum> : Op<T, kSum> {};

template <typename T> struct Scale;
template <> struct Scale<float> {
  __device__ static float f(u64 s, float x) {
#pragma clang fp contract(off)
    return __uint_as_float((uint32_t)s) * x;
  }
};
template <> struct Scale<double> {
  __device__ static double f(u64 s, double x) {
#pragma clang fp contract(off)
    return __longlong_as_double((long long)s) * x;
  }
};
template <> struct Scale<_Float16> {
  __device__ static _Float16 f(u64 s, _Float16 x) {
#pragma clang fp contract(off)
    return __builtin_bit_cast(_Float16, (uint16_t)s) * x;
  }
};
template <> struct Scale<bf16_t> {
  __device__ static bf16_t f(u64 s, bf16_t x) {
#pragma clang fp contract(off)
    bf16_t sb;
    sb.v = (uint16_t)s;
    return f2bf(bf2f(sb) * bf2f(x));
  }
};
template <> struct Scale<int32_t> {
  __device__ static int32_t f(u64 s, int32_t x) { return (int32_t)((uint32_t)s * (uint32_t)x); }
};

// fp8: the scalar is one fp8 byte; y = encode(float(s) * float(x)), the product exact in f32
template <> struct Scale<e4m3_t> {
  __device__ static e4m3_t f(u64 s, e4m3_t x) {
    e4m3_t r;
    r.v = (uint8_t)fp8_scale2<e4m3_t, false>((uint32_t)s, x.v, 0u);
    return r;
  }
};
template <> struct Scale<e5m2_t> {
  __device__ static e5m2_t f(u64 s, e5m2_t x) {
    e5m2_t r;
    r.v = (uint8_t)fp8_scale2<e5m2_t, false>((uint32_t)s, x.v, 0u);
    return r;
  }
};

template <typename T> struct alignas(16) Pack16 { T x[16 / sizeof(T)]; };

// an input on its way into a fold: scaled for kPreMulSum, untouched (and no code) for every other op
template <typename T, int OPC>
__device__ __forceinline__ T prescale(T x, u64 s) {
  if constexpr (OPC == kPreMulSum) return Scale<T>::f(s, x);
  else return x;
}
template <typename T, int OPC>
__device__ __forceinline__ v4u prescale16(v4u a, u64 s) {
  if constexpr (OPC == kPreMulSum && IsFp8<T>::value) {
    // (fp8: dword by dword, so that two elements share each conversion)
    v4u r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fp8_scale2<T, true>((uint32_t)s, a[i], fp8_scale2<T, false>((uint32_t)s, a[i], 0u));
    return r;
  } else if constexpr (OPC == kPreMulSum) {
    Pack16<T> pa = __builtin_bit_cast(Pack16<T>, a);
#pragma unroll
    for (int i = 0; i < (int)(16 / sizeof(T)); ++i) pa.x[i] = Scale<T>::f(s, pa.x[i]);
    return __builtin_bit_cast(v4u, pa);
  } else {
    return a;
  }
}

template <typename T, int OPC>
__device__ __forceinline__ v4u reduce16(v4u a, v4u b) {
  if constexpr (IsFp8<T>::value) {
    // 16 elements, dword by dword: two elements per conversion each way (8 + 8 in, 8 out)
    v4u r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = fp8_fold4<T, OPC == kPreMulSum ? kSum : OPC>(a[i], b[i]);
    return r;
  } else {
    Pack16<T> pa = __builtin_bit_cast(Pack16<T>, a);
    const Pack16<T> pb = __builtin_bit_cast(Pack16<T>, b);
#pragma unroll
    for (int i = 0; i < (int)(16 / sizeof(T)); ++i) pa.x[i] = Op<T, OPC>::f(pa.x[i], pb.x[i]);
    return __builtin_bit_cast(v4u, pa);
  }
}

// ---------------------------------------------------------------- memory primitives
__device__ __forceinline__ u64 ld_sys(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint32_t ld_sys32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys(u64* p, u64 v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void st_sys32(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ v4u ld_slot16(rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kAuxSys);
}
__device__ __forceinline__ void st_slot16(rsrc_t r, uint32_t off, v4u v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kAuxSys);
}
// non-temporal buffer access (this rank's own bytes in the read kernel's short-slice forms:
// out-of-range lanes of a buffer access read 0 and write nothing, so those loops need no
// per-lane predicate)
constexpr int kAuxNt = 2;
__device__ __forceinline__ v4u ld_nt16(rsrc_t r, uint32_t off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kAuxNt);
}
__device__ __forceinline__ void st_nt16(rsrc_t r, uint32_t off, v4u v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, kAuxNt);
}
// this rank's own send / recv bytes are touched once per call: non-temporal (see local reduce)
__device__ __forceinline__ v4u ld_g16(const char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
}
__device__ __forceinline__ void st_g16(char* p, v4u v) { __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(p)); }

// scalar (unaligned-count) path: one element per access
template <int SZ> struct Scal;
template <> struct Scal<1> {
  typedef uint8_t U;
  __device__ static U ld(rsrc_t r, uint32_t o) { return __builtin_amdgcn_raw_buffer_load_b8(r, o, 0, kAuxSys); }
  __device__ static void st(rsrc_t r, uint32_t o, U v) { __builtin_amdgcn_raw_buffer_store_b8(v, r, o, 0, kAuxSys); }
};
template <> struct Scal<2> {
  typedef uint16_t U;
  __device__ static U ld(rsrc_t r, uint32_t o) { return __builtin_amdgcn_raw_buffer_load_b16(r, o, 0, kAuxSys); }
  __device__ static void st(rsrc_t r, uint32_t o, U v) { __builtin_amdgcn_raw_buffer_store_b16(v, r, o, 0, kAuxSys); }
};
template <> struct Scal<4> {
  typedef uint32_t U;
  __device__ static U ld(rsrc_t r, uint32_t o) { return __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, kAuxSys); }
  __device__ static void st(rsrc_t r, uint32_t o, U v) { __builtin_amdgcn_raw_buffer_store_b32(v, r, o, 0, kAuxSys); }
};
template <> struct Scal<8> {
  typedef u64 U;
  __device__ static U ld(rsrc_t r, uint32_t o) {
    auto v = __builtin_amdgcn_raw_buffer_load_b64(r, o, 0, kAuxSys);
    return __builtin_bit_cast(U, v);
  }
  __device__ static void st(rsrc_t r, uint32_t o, U v) {
    typedef unsigned int v2u __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, o, 0, kAuxSys);
  }
};

// message `seq` from `src` to `dst` on pipeline w: in the receiver's scratch (schedule.h
// msg_slot_off); peer_scratch[rank] is this rank's own scratch
__device__ __forceinline__ char* msg_slot(const CollParams& p, int C, int src, int dst, int w, u64 seq) {
  return p.peer_scratch[dst] + msg_slot_off(C, p.nslots, p.slot_bytes, src, dst, w, seq);
}

// ---------------------------------------------------------------- bounded waits
struct Ctl {
  uint32_t* status;
  const uint32_t* host_abort;
  const u64* my_abort;
  uint64_t timeout_ticks;
  const u64* mbox;   // this rank's mailbox base (for the timeout diagnostic)
  uint32_t* claim;   // device word: the first give-up of the communicator takes it (claim_first)
};

// The first give-up -- a timeout, a peer's ABORT, the host's abort -- of any lane of any wave
// claims the status with one agent-scope compare-and-swap on a device word (the host-mapped
// status page itself takes no atomics: no PCIe atomics needed), so the cause and the diagnostic
// the host reports come from ONE lane: lanes of wave_wait_peers that give up in the same round,
// or a timeout racing a peer's ABORT, can no longer mix their words or overwrite the first cause
// (ADVICE r4).  The winner writes its words, then the status; the others just give up.
__device__ __forceinline__ bool claim_first(const Ctl& c) {
  uint32_t expected = 0;
  return __hip_atomic_compare_exchange_strong(c.claim, &expected, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
}

// a timed-out wait: which mailbox word, the target and the last value seen (host-mapped words
// 4..6 of the control page, plain system-scope stores), then the status
__device__ __forceinline__ void record_timeout(const Ctl& c, const u64* flag, u64 target, u64 seen) {
  if (!claim_first(c)) return;
  u64* diag = reinterpret_cast<u64*>(c.status + 4);
  __hip_atomic_store(diag + 0, (u64)(flag - c.mbox), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(diag + 1, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(diag + 2, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  st_sys32(c.status, kStatusTimeout);
}

// a peer's ABORT word seen: recorded only as the first cause (a peer's abort that echoes this
// rank's own timeout must not hide it); the word names the peer and its cause
__device__ __forceinline__ void note_remote_abort(const Ctl& c, u64 a) {
  if (!claim_first(c)) return;
  __hip_atomic_store(reinterpret_cast<u64*>(c.status + 4) + 3, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  st_sys32(c.status, kStatusRemoteAbort);
}

// lane-0 spin until *flag >= target; false on timeout / abort (status already set).  The
// spin is out of line (kept out of the message bodies' code and registers); Ctl goes by value
// so it travels in registers -- by reference it had to live in scratch memory.
#ifndef MNCCL_POLL_SLEEP
#define MNCCL_POLL_SLEEP 1  // s_sleep units (64 clocks each) between two polls of a flag
#endif
__device__ __noinline__ bool wait_ge_spin(const u64* flag, u64 target, const Ctl c) {
  const u64 t0 = __builtin_amdgcn_s_memrealtime();
  for (uint32_t polls = 1;; ++polls) {
    __builtin_amdgcn_s_sleep(MNCCL_POLL_SLEEP);
    if (ld_sys(flag) >= target) return true;
    if ((polls & 63) == 0) {
      if (const u64 a = ld_sys(c.my_abort)) {
        note_remote_abort(c, a);
        return false;
      }
      if (ld_sys32(c.host_abort) != 0) {
        if (claim_first(c)) st_sys32(c.status, kStatusHostAbort);
        return false;
      }
      if (ld_sys32(c.status) != 0) return false;  // a sibling workgroup gave up
      if (__builtin_amdgcn_s_memrealtime() - t0 > c.timeout_ticks) {
        record_timeout(c, flag, target, ld_sys(flag));
        return false;
      }
    }
  }
}

// the common case (the flag is already there) costs one load and no call
__device__ __forceinline__ bool wait_ge(const u64* flag, u64 target, const Ctl& c) {
  if (ld_sys(flag) >= target) return true;
  return wait_ge_spin(flag, target, c);
}

// After a READY poll.  Every load of handed-off bytes is an sc0 sc1 buffer load of uncached
// scratch (never L1/L2 resident) and every producer stored them sc0 sc1 and drained before its
// flag (cdna_hip_programming.md G16 "sc1 loads replace the acquire"), so with
// MINI_NCCL_SYS_FENCE=0 the fence is only a compiler barrier; =1 keeps the system acquire.
__device__ __forceinline__ void acquire_sys(int sys_fence) {
  if (sys_fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// every storing wave: drain its stores (asm so the compiler cannot elide it)
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// lane 0, after its wave's drain
__device__ __forceinline__ void publish(u64* flag, u64 v, int sys_fence) {
  if (sys_fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  st_sys(flag, v);
}

// ---------------------------------------------------------------- wave-level sync
// A channel is ONE wave (64 lanes): lane 0 polls and signals, the wave's own s_waitcnt orders
// its memory operations, and no workgroup barrier is ever needed -- the waves of a
// workgroup (one by default) are independent pipelines.
__device__ __forceinline__ bool wave_wait_ge(const u64* flag, u64 target, const Ctl& c, int lane) {
  int ok = 1;
  if (lane == 0) ok = wait_ge(flag, target, c) ? 1 : 0;
  return __builtin_amdgcn_readfirstlane(ok) != 0;
}

// Lane l waits for its own word (the peers' READY / CREDIT / DONE words, one lane per peer):
// every peer's flag is polled in the same round instead of one peer after the other (n - 1
// uncached round trips in a row at every hand-off of the read and one-shot kernels).  True when
// every active lane's word arrived; a lane that gives up sets the status as wait_ge does.
// check_abort: lane 63 (never a peer's: at most 16 ranks) also reads this rank's ABORT word in
// the same round -- a wait whose flags are all there already never spins, so without it a rank
// that comes late to a call its peer gave up on (the peer raised its ABORT word, its messages
// already sent) would complete the call as if nothing had happened.
__device__ __forceinline__ bool wave_wait_peers(const u64* flag, u64 target, bool active, const Ctl& c, int lane,
                                                bool check_abort) {
  int bad = 0;
  if (active) {
    bad = wait_ge(flag, target, c) ? 0 : 1;
  } else if (check_abort && lane == 63) {
    if (const u64 a = ld_sys(c.my_abort)) {
      note_remote_abort(c, a);
      bad = 1;
    }
  }
  return __builtin_amdgcn_ballot_w64(bad != 0) == 0;
}

// Registered-window calls (Comm::allreduce's fast path) are launched without a host rendezvous: the
// peers' buffer addresses come from the windows every rank registered together, on the promise
// that every rank passes the same windows, offsets, count, dtype and op.  The promise is checked
// here, on the device, before any peer buffer is touched: START carries the caller's signature
// (a hash of those, never 0) in word kSigWord of the READY line, stored just before the flag (no
// drain between the two: the signature may land after the flag).  After every peer's START, lane
// q waits for peer q's signature word to be non-zero, compares it with this rank's and clears it
// (so a later call never meets a stale one: a peer writes its next signature only after this
// call's DONE).  Any difference -- seen by every rank alike, as every rank compares every pair it
// is part of -- gives up the call with kStatusMismatch (ncclInvalidUsage).
// The START of read_start_kernel; read_kernel writes the same stores inline, its flag value read
// inside the peer-lane branch (read outside it, from a clamped LDS index, the persistent kernel's
// fold spilled 36 registers to scratch at the 256-register bound).
__device__ __forceinline__ void send_start(const CollParams& p, int C, int lane, u64 v, int w) {
  const int n = p.n, r = p.rank;
  if (lane < n && lane != r && p.sig) st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w) + kSigWord, p.sig);
  if (lane < n && lane != r) st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), v);
}

// lane q: does peer q's signature differ from mine?  Clears the word.  Out of line: kept out of
// the persistent kernel's register allocation, whose fold sits at the 256-register bound
__device__ __noinline__ bool sig_differs(u64* word, u64 sig) {
  const bool bad = ld_sys(word) != sig;
  st_sys(word, 0);
  return bad;
}

// after every peer's START: false (status claimed, nothing touched) if some peer's signature differs.
// *seen: kStatusMismatch when this wave saw the difference itself -- its ABORT word then carries
// that cause even if another wave won the claim and its status store has not landed yet (ADVICE
// r5: re-reading the shared status could send a bare abort, and the peer report ncclRemoteError)
__device__ __forceinline__ bool starts_agree(const CollParams& p, const Ctl& c, int C, int lane, int w,
                                             uint32_t* seen) {
  if (!p.sig) return true;
  const int n = p.n, r = p.rank;
  const bool peer = lane < n && lane != r;
  u64* word = p.mbox + mbox_ready(C, peer ? lane : 0, w) + kSigWord;
  if (!wave_wait_peers(word, 1, peer, c, lane, false)) return false;  // (status set: timeout / abort)
  bool bad = false;
  if (peer) bad = sig_differs(word, p.sig);
  if (__builtin_amdgcn_ballot_w64(bad) == 0) return true;
  *seen = kStatusMismatch;
  if (lane == 0 && claim_first(c)) st_sys32(c.status, kStatusMismatch);
  return false;
}

// ---------------------------------------------------------------- message bodies (one wave)
enum : int { kHasLocal = 1, kHasIn = 2, kWritesRecv = 4, kSends = 8, kReduces = 16 };
template <int KIND> struct KindBits;
template <> struct KindBits<kSend> { static constexpr int v = kHasLocal | kSends; };
template <> struct KindBits<kReduceSend> { static constexpr int v = kHasLocal | kHasIn | kSends | kReduces; };
template <> struct KindBits<kReduceCopySend> { static constexpr int v = kHasLocal | kHasIn | kSends | kReduces | kWritesRecv; };
template <> struct KindBits<kCopySend> { static constexpr int v = kHasIn | kSends | kWritesRecv; };
template <> struct KindBits<kCopy> { static constexpr int v = kHasIn | kWritesRecv; };
template <> struct KindBits<kForward> { static constexpr int v = kHasIn | kSends; };  // (kDrop moves nothing)

constexpr int kU = 8;  // 16-byte vectors per lane per batch: 8 KiB per wave in flight per stream

template <typename T, int OPC, int KIND>
__device__ __forceinline__ void vec_one(const char* lsrc, char* ldst, rsrc_t in, rsrc_t out, uint32_t i, u64 sc) {
  constexpr int B = KindBits<KIND>::v;
  v4u l, x, v;
  // (the local operand is this rank's input: kPreMulSum scales it here, prescale16)
  if (B & kHasLocal) l = prescale16<T, OPC>(ld_g16(lsrc + (size_t)i * 16), sc);
  if (B & kHasIn) x = ld_slot16(in, i * 16);
  if (B & kReduces) v = reduce16<T, OPC>(l, x);
  else if (B & kHasIn) v = x;
  else v = l;
  if (B & kWritesRecv) st_g16(ldst + (size_t)i * 16, v);
  if (B & kSends) st_slot16(out, i * 16, v);
}

template <typename T, int OPC, int KIND>
__device__ __forceinline__ void move_scalar(const char* __restrict__ lsrc, char* __restrict__ ldst, rsrc_t in,
                                            rsrc_t out, uint32_t nbytes, int lane, uint32_t off0, u64 sc);

// 16-byte vectors over the message, then its last (nbytes % 16) bytes element by element.
// The local side (send / recv) may be element- but not 16-byte-aligned (4-byte-aligned
// dwordx4 accesses are valid on gfx950); the slot side is always 16-byte-aligned.
template <typename T, int OPC, int KIND, int UB = kU>
__device__ __forceinline__ void move_vec(const char* __restrict__ lsrc, char* __restrict__ ldst, rsrc_t in,
                                         rsrc_t out, uint32_t nbytes, int lane, u64 sc) {
  constexpr int B = KindBits<KIND>::v;
  const uint32_t nvec = nbytes >> 4;
  uint32_t b = 0;
  for (; b + 64 * UB <= nvec; b += 64 * UB) {  // full batches: every lane issues UB loads per stream
    v4u l[UB], x[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const uint32_t i = b + (uint32_t)(u * 64 + lane);
      if (B & kHasLocal) l[u] = ld_g16(lsrc + (size_t)i * 16);
      if (B & kHasIn) x[u] = ld_slot16(in, i * 16);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const uint32_t i = b + (uint32_t)(u * 64 + lane);
      v4u v;
      if (B & kHasLocal) l[u] = prescale16<T, OPC>(l[u], sc);
      if (B & kReduces) v = reduce16<T, OPC>(l[u], x[u]);
      else if (B & kHasIn) v = x[u];
      else v = l[u];
      if (B & kWritesRecv) st_g16(ldst + (size_t)i * 16, v);
      if (B & kSends) st_slot16(out, i * 16, v);
    }
  }
  for (uint32_t i = b + (uint32_t)lane; i < nvec; i += 64) vec_one<T, OPC, KIND>(lsrc, ldst, in, out, i, sc);
  if (nbytes & 15u) move_scalar<T, OPC, KIND>(lsrc, ldst, in, out, nbytes, lane, nvec * 16, sc);
}

// elements [off0 / sizeof(T), nbytes / sizeof(T)) of the message, one per lane
template <typename T, int OPC, int KIND>
__device__ __forceinline__ void move_scalar(const char* __restrict__ lsrc, char* __restrict__ ldst, rsrc_t in,
                                            rsrc_t out, uint32_t nbytes, int lane, uint32_t off0, u64 sc) {
  constexpr int B = KindBits<KIND>::v;
  typedef typename Scal<sizeof(T)>::U U;
  const uint32_t ne = nbytes / sizeof(T);
  for (uint32_t i = off0 / sizeof(T) + lane; i < ne; i += 64) {
    U l = 0, x = 0, v;
    if (B & kHasLocal) l = __builtin_bit_cast(U, prescale<T, OPC>(reinterpret_cast<const T*>(lsrc)[i], sc));
    if (B & kHasIn) x = Scal<sizeof(T)>::ld(in, i * (uint32_t)sizeof(T));
    if (B & kReduces) v = __builtin_bit_cast(U, Op<T, OPC>::f(__builtin_bit_cast(T, l), __builtin_bit_cast(T, x)));
    else if (B & kHasIn) v = x;
    else v = l;
    if (B & kWritesRecv) reinterpret_cast<U*>(ldst)[i] = v;
    if (B & kSends) Scal<sizeof(T)>::st(out, i * (uint32_t)sizeof(T), v);
  }
}

template <typename T, int OPC, bool VEC, int KIND, int UB = kU>
__device__ __forceinline__ void move(const char* lsrc, char* ldst, rsrc_t in, rsrc_t out, uint32_t nbytes, int lane,
                                     u64 sc = 0) {
  if (VEC) move_vec<T, OPC, KIND, UB>(lsrc, ldst, in, out, nbytes, lane, sc);
  else move_scalar<T, OPC, KIND>(lsrc, ldst, in, out, nbytes, lane, 0, sc);
}

// the ABORT word a giving-up rank writes into its peers' mailboxes: its rank + 1 (never 0) and
// its own status (why it gave up), plus the cause this wave saw itself (`seen`) -- the peers
// report both (Comm::check_status)
__device__ __forceinline__ u64 abort_word(const CollParams& p, uint32_t seen = 0) {
  return ((u64)(ld_sys32(p.status) | seen) << 32) | (u64)(p.rank + 1);
}

__device__ __forceinline__ void abort_peers(const CollParams& p, int C, int a, int b) {
  st_sys(p.peer_mbox[a] + mbox_abort(p.n, C), abort_word(p));
  st_sys(p.peer_mbox[b] + mbox_abort(p.n, C), abort_word(p));
}

// the host watchdog's deadline starts when the kernel does (Comm::wait_for): one posted write
__device__ __forceinline__ void signal_start(const CollParams& p) {
  if (blockIdx.x == 0 && threadIdx.x == 0) st_sys32(p.started, p.call_seq);
}

// The count % n elements past the chunks keep this rank's own input (api.cpp:173-175 copies the
// whole buffer, mini_nccl.cu:69 never touches the tail): pipeline 0 copies them, byte by byte
// (under 128 bytes), so a call is one launch.  Measured on the one-GPU box: a copy kernel queued
// in front of a persistent kernel can find no room left by the co-located ranks' persistent
// kernels, which then wait for this rank's forever (tools/dr_probe.py,
// profiles/r3_device_rendezvous.txt: 2 of 2 runs stalled with the copy, 4 of 4 clean without).
__device__ __forceinline__ void copy_tail(const CollParams& p, int w, int lane) {
  if (w != 0 || p.tail_bytes == 0) return;
  const uint64_t off = p.chunk_bytes * (uint64_t)p.n;
  for (uint64_t i = (uint64_t)lane; i < p.tail_bytes; i += 64) p.recv[off + i] = p.send[off + i];
}

// channel geometry: one channel per wave
struct WaveId {
  int lane, wv, w, C;
};
__device__ __forceinline__ WaveId wave_id() {
  WaveId id;
  id.lane = threadIdx.x & 63;
  const int W = blockDim.x >> 6;
  id.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  id.w = __builtin_amdgcn_readfirstlane(blockIdx.x * W + id.wv);
  id.C = gridDim.x * W;
  return id;
}

// ---------------------------------------------------------------- ring kernel
// Every rank's persistent kernel waits for its peers' kernels, so on a GPU that several rank
// processes share (the reference's perf_test topology, the one-GPU test box) all of them must be
// resident at once: 8 ranks x 256 one-wave pipelines = 2 waves on each of the 1024 SIMDs.  The
// collective kernels therefore ask for >= 2 waves per SIMD (<= 256 VGPRs + AGPRs per wave; a
// read-kernel variant at 256 + 1 AGPR fitted only one, and 8 co-located ranks crawled until
// their watchdogs fired).  With one rank per GPU this costs nothing.  (kernels.h
// kMinWavesPerSimd; Comm caps a call's pipelines so that every rank's waves fit, Comm::run_pipes.)

// The kernels that fold have their code in a *_body function and two entry points: the one named
// for the four built-in ops, and a `scaled_*` one for kPreMulSum (the resource budget of the
// built-in kernels is checked by name, tests/test_kernel_resources.py; the scaled ones have the
// same budget, tests/test_premul_cpu.py).  (__restrict__: the argument is the kernel's own copy; without
// it the ring kernels took one register more than they had as kernels of their own.)
template <typename T, int OPC, bool VEC>
__device__ __forceinline__ void ring_body(const CollParams& __restrict__ p) {
  signal_start(p);
  const WaveId id = wave_id();
  // C: the communicator's pipelines (mailbox, scratch and counter layout); A: the ones this call
  // runs (its grid, schedule.h call_pipelines), slice s on pipeline s mod A
  const int lane = id.lane, w = id.w, C = p.pipes, A = id.C;
  const int n = p.n, r = p.rank, K = p.nslots;
  copy_tail(p, w, lane);
  const int prev = mod_n(r - 1, n), next = mod_n(r + 1, n);
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  // per-pair message counters: the FIFO to `next` and the FIFO from `prev` on this channel
  u64* tx_ctr = p.tx_seq + (u64)next * C + w;
  u64* rx_ctr = p.rx_seq + (u64)prev * C + w;
  const u64 tx_base = *tx_ctr, rx_base = *rx_ctr;
  // the op table of the call's collective (schedule.h coll_op: the all-reduce's ring, one of its
  // halves for ncclReduceScatter / ncclAllGather, the chain of ncclBroadcast or the masked ring of
  // ncclReduce); each link's counters advance by what the link carried (Broadcast's root-1 -> root
  // carries nothing: coll_tx_msgs / coll_rx_msgs, the same value everywhere else)
  const int coll = p.coll, root = p.root;
  const int mpi_tx = coll_tx_msgs(coll, n, r, root), mpi_rx = coll_rx_msgs(coll, n, r, root);
  const u64* my_ready = p.mbox + mbox_ready(C, prev, w);
  const u64* my_credit = p.mbox + mbox_credit(n, C, next, w);
  u64* out_ready = p.peer_mbox[next] + mbox_ready(C, r, w);
  u64* out_credit = p.peer_mbox[prev] + mbox_credit(n, C, r, w);
  const int nops = coll_num_ops(coll, n, r, root);  // (gather / scatter: by the rank's place in the chain)

  for (uint32_t it = 0; it < p.iters; ++it) {
    const u64 s = (u64)it * A + w;
    const uint32_t len0 = (uint32_t)slice_len(p.chunk_bytes, p.slice_bytes, s);
    const u64 soff = s * p.slice_bytes;
    for (int k = 0; k < nops; ++k) {
      const RingOp o = coll_op(coll, n, r, k, root);
      const u64 rseq = rx_base + (u64)it * mpi_rx + (u64)o.recv_msg, sseq = tx_base + (u64)it * mpi_tx + (u64)o.send_msg;
      // ncclReduce: the trailing chunks may be short or empty (every rank clamps chunk o.chunk alike;
      // an empty message still moves its flags)
      const uint32_t len = coll == kCollReduce ? (uint32_t)rooted_len(p.total_bytes, (u64)o.chunk * p.chunk_bytes,
                                                                      p.chunk_bytes, p.slice_bytes, s)
                                               : len0;
      bool ok = true;
      if (o.recv_msg >= 0) ok = wave_wait_ge(my_ready, rseq + 1, ctl, lane);
      if (ok && o.send_msg >= 0 && sseq + 1 > (u64)K) ok = wave_wait_ge(my_credit, sseq + 1 - K, ctl, lane);
      if (!ok) {
        if (lane == 0) abort_peers(p, C, prev, next);
        return;
      }
      if (o.recv_msg >= 0) acquire_sys(p.sys_fence);
      if (len && o.kind != kDrop) {
        const u64 coff = (u64)o.chunk * p.chunk_bytes + soff;
        const rsrc_t in = make_rsrc(msg_slot(p, C, prev, r, w, rseq), len);
        const rsrc_t out = make_rsrc(msg_slot(p, C, r, next, w, sseq), len);
        const char* lsrc = p.send + coff;
        char* ldst = p.recv + coff;
        switch (o.kind) {
          case kSend: move<T, OPC, VEC, kSend>(lsrc, ldst, in, out, len, lane, p.scale); break;
          case kReduceSend: move<T, OPC, VEC, kReduceSend>(lsrc, ldst, in, out, len, lane, p.scale); break;
          case kReduceCopySend: move<T, OPC, VEC, kReduceCopySend>(lsrc, ldst, in, out, len, lane, p.scale); break;
          case kCopySend: move<T, OPC, VEC, kCopySend>(lsrc, ldst, in, out, len, lane, p.scale); break;
          case kForward: move<T, OPC, VEC, kForward>(lsrc, ldst, in, out, len, lane, p.scale); break;
          default: move<T, OPC, VEC, kCopy>(lsrc, ldst, in, out, len, lane, p.scale); break;
        }
      }
      drain_stores();  // every load of the slot has returned and every store has landed
      if (lane == 0) {
        if (o.send_msg >= 0) publish(out_ready, sseq + 1, p.sys_fence);
        if (o.recv_msg >= 0) st_sys(out_credit, rseq + 1);
      }
    }
  }
  if (lane == 0) {
    *tx_ctr = tx_base + (u64)p.iters * mpi_tx;
    *rx_ctr = rx_base + (u64)p.iters * mpi_rx;
  }
}

template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) ring_kernel(CollParams p) {
  ring_body<T, OPC, VEC>(p);
}
template <typename T, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scaled_ring(CollParams p) {
  ring_body<T, kPreMulSum, VEC>(p);
}
// The fp8 types' entry points (the `fp8_*` family: the built-in kernels' instantiation sets are
// pinned by name and count, so the one-byte types get names of their own over the same bodies, as
// kPreMulSum got scaled_*); OPC: the four built-in ops and kPreMulSum.
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) fp8_ring(CollParams p) {
  ring_body<T, OPC, VEC>(p);
}

constexpr int kMaxWaves = kMaxThreads / 64;

// ---------------------------------------------------------------- read kernel
// MINI_NCCL_ALGO=read (schedule.h): no scratch.  Comm maps every peer's send and recv buffers
// (dma-buf imports, negotiated per call); rank r folds slice s of its own chunk r straight from
// the peers' send buffers (sc0 sc1 loads over the links, in ring order) and stores the result
// into its own recv and into every peer's recv with sc0 sc1 stores (the push form; 4.0-5.x also
// built a load form, every peer copying the result out of the owner's recv after a READY: 1.1-1.45x
// slower everywhere it was measured, removed in 6.0).
//
// Fold of slice `nbytes` at byte `coff` of chunk r: acc = op(x_q, acc) in ring order.
template <typename T, int OPC>
__device__ __forceinline__ void read_fold_scalar(const CollParams& p, uint64_t coff, uint32_t nbytes, int lane,
                                                 uint32_t off0) {
  const int n = p.n, r = p.rank;
  typedef typename Scal<sizeof(T)>::U Us;
  const rsrc_t out = make_rsrc(p.recv + coff, nbytes);
  const uint32_t ne = nbytes / sizeof(T);
  for (uint32_t i = off0 / sizeof(T) + lane; i < ne; i += 64) {
    T acc = prescale<T, OPC>(reinterpret_cast<const T*>(p.send + coff)[i], p.scale);
    for (int k = 1; k < n; ++k) {
      const rsrc_t in = make_rsrc(p.peer_send[direct_peer(n, r, k)] + coff, nbytes);
      acc = Op<T, OPC>::f(prescale<T, OPC>(__builtin_bit_cast(T, Scal<sizeof(T)>::ld(in, i * (uint32_t)sizeof(T))), p.scale), acc);
    }
    Scal<sizeof(T)>::st(out, i * (uint32_t)sizeof(T), __builtin_bit_cast(Us, acc));
  }
}

// Vectors per lane per batch of the read kernel's fold past 8 ranks: 16 (two peers' 16 KiB in
// flight per wave).  Latency insurance for loads that cross xGMI: a wave's rate is its bytes in
// flight over the load's round trip, so twice the scratch kernels' batches halve the pipelines a
// link needs to stay busy; measured free on the one-GPU proxy (profiles/r2_read_batch_variants.txt).
#ifndef MNCCL_READ_FOLD_U
#define MNCCL_READ_FOLD_U 16
#endif
constexpr int kReadFoldU = MNCCL_READ_FOLD_U;

// Short slices (below one full batch, and the part of a slice past its full batches): every
// peer's vectors of a step are loaded at once -- (n-1) x kWideV KiB in flight per wave -- so a
// step costs one load round trip, where a peer-by-peer loop of single vectors cost one per peer
// and vector (a 1 KiB slice over 7 peers: 1 round trip instead of 7 in the fold, and in the
// copy).  The buffer resources end at the slice's last whole vector: lanes past it load 0 and
// store nothing (no predicate, so no load waits on another); the last nbytes % 16 bytes go
// element by element as before.
constexpr int kWideV = 2;
constexpr int kWideG = 7;  // peers per group (a node's n - 1): their buffer descriptors stay in SGPRs

template <typename T, int OPC>
__device__ __forceinline__ void read_fold_wide(const CollParams& p, uint64_t coff, uint32_t vlo, uint32_t nvec,
                                               int lane) {
  const int n = p.n, r = p.rank;
  const uint32_t vb = nvec * 16;
  const rsrc_t loc = make_rsrc(p.send + coff, vb), out = make_rsrc(p.recv + coff, vb);
  for (uint32_t b = vlo; b < nvec; b += 64 * kWideV) {
    v4u acc[kWideV];
#pragma unroll
    for (int u = 0; u < kWideV; ++u) acc[u] = ld_nt16(loc, (b + (uint32_t)(u * 64 + lane)) * 16);
#pragma unroll
    for (int u = 0; u < kWideV; ++u) acc[u] = prescale16<T, OPC>(acc[u], p.scale);
    for (int k0 = 1; k0 < n; k0 += kWideG) {  // ring order: groups in turn, peers in turn
      v4u x[kWideG][kWideV];
#pragma unroll
      for (int g = 0; g < kWideG; ++g)
        if (k0 + g < n) {
          const rsrc_t in = make_rsrc(p.peer_send[direct_peer(n, r, k0 + g)] + coff, vb);
#pragma unroll
          for (int u = 0; u < kWideV; ++u) x[g][u] = ld_slot16(in, (b + (uint32_t)(u * 64 + lane)) * 16);
        }
#pragma unroll
      for (int g = 0; g < kWideG; ++g)
        if (k0 + g < n) {
#pragma unroll
          for (int u = 0; u < kWideV; ++u) acc[u] = reduce16<T, OPC>(prescale16<T, OPC>(x[g][u], p.scale), acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < kWideV; ++u) st_slot16(out, (b + (uint32_t)(u * 64 + lane)) * 16, acc[u]);
  }
}

// The fold of a slice from 4 to 8 ranks (a node): each batch loads V vectors per lane from EVERY
// peer at once, and the next batch's loads leave before this batch is folded (two register
// sets).  The fold's order is fixed (ring order), its load order is not: loaded one peer after
// the other, every wave of every rank would start its batches at peer r+1 and the ranks'
// incoming traffic would sit on one link at a time -- over xGMI, a seventh of a rank's links
// at 8 ranks; loaded together, every link carries its share all the time.  G peer slots, V
// vectors: (n-1) x V KiB per batch, two batches in flight per wave (2 ranks: 12 KiB, 3: 8 KiB
// per peer, 4-5: 4 KiB, 6-8: 3 KiB; all within 256 registers without spilling).  Measured on
// the one-GPU proxy against the one-peer-ahead batches below (used past 8 ranks): equal at 2
// and 3 ranks (profiles/r2_read_fold_all_n23_ab.txt), 0.94-1.05x at 4 and 8.
//
// The read schedule's second half: each rank pushes its result slices into every peer's recv
// (sc0 sc1 stores, straight from the fold's registers) -- no per-iteration READY, no copy phase,
// and each GPU's HBM moves 2n chunks per call (a load form, every peer reading the result back
// from the owner's recv, moved 3n-1 and was 1.1-1.45x slower: profiles/r3_read_push_ab.txt); DONE
// also means "my pushes into your recv have landed", and every rank waits for every peer's DONE
// before its kernel ends.  Only rank r ever writes chunk r of any recv (in place: after its own
// loads of that slice).  The pushes are sc0 sc1 stores: each is acknowledged once it reached the
// owner's memory, which drops any copy of the line the owner's L2 kept (file header), and this
// rank never reads the pushed ranges inside the call.
//
// The fold's store into p.recv is sc0 sc1 like the pushes.  No peer reads this rank's OWN recv
// inside the call, so there it could be non-temporal, as the local reduce's is: measured equal
// within the spread and not shipped (profiles/r6_own_nt_store_ab.txt).
// PUSH = false (scatter_fold, ncclReduceScatter): the same fold stored into p.recv only.  For
// root_fold (ncclReduce) p.recv is the ROOT's recv, another agent's memory on every rank but the
// root: there the one store is a push and has to be sc0 sc1.
template <typename T, int OPC, int G, int V, bool PUSH = true>
__device__ __forceinline__ void read_fold_all(const CollParams& p, uint64_t coff, uint32_t nvec, int lane) {
  constexpr uint32_t step = 64 * V;
  const int n = p.n, r = p.rank, w = wave_id().w;
  const uint32_t vb = nvec * 16;
  const rsrc_t loc = make_rsrc(p.send + coff, vb), out = make_rsrc(p.recv + coff, vb);
  rsrc_t in[G];
#pragma unroll
  for (int g = 0; g < G; ++g) in[g] = make_rsrc(p.peer_send[direct_peer(n, r, 1 + (g + 1 < n ? g : 0))] + coff, vb);
  // the result also goes to the same offset of every peer's recv (pipeline w starts at peer
  // w mod n-1, so a rank's pipelines spread their pushes over all links)
  rsrc_t pout[PUSH ? G : 1];
#pragma unroll
  for (int g = 0; g < (PUSH ? G : 0); ++g)
    pout[g] = make_rsrc(p.peer_recv[direct_peer(n, r, 1 + (g + 1 < n ? (g + w) % (n - 1) : 0))] + coff, vb);
  v4u xa[G][V], aa[V], xb[G][V], ab[V];
  auto load = [&](v4u(&x)[G][V], v4u(&a)[V], uint32_t b) {
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (g + 1 < n) {
#pragma unroll
        for (int u = 0; u < V; ++u) x[g][u] = ld_slot16(in[g], (b + (uint32_t)(u * 64 + lane)) * 16);
      }
#pragma unroll
    for (int u = 0; u < V; ++u) a[u] = ld_nt16(loc, (b + (uint32_t)(u * 64 + lane)) * 16);
  };
  auto fold_store = [&](v4u(&x)[G][V], v4u(&a)[V], uint32_t b) {
    // (kPreMulSum: every operand is some rank's input -- the own slice and every peer's are scaled)
#pragma unroll
    for (int u = 0; u < V; ++u) a[u] = prescale16<T, OPC>(a[u], p.scale);
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (g + 1 < n) {
#pragma unroll
        for (int u = 0; u < V; ++u) a[u] = reduce16<T, OPC>(prescale16<T, OPC>(x[g][u], p.scale), a[u]);
      }
#pragma unroll
    for (int u = 0; u < V; ++u) st_slot16(out, (b + (uint32_t)(u * 64 + lane)) * 16, a[u]);
#pragma unroll
    for (int g = 0; g < (PUSH ? G : 0); ++g)
      if (g + 1 < n) {
#pragma unroll
        for (int u = 0; u < V; ++u) st_slot16(pout[g], (b + (uint32_t)(u * 64 + lane)) * 16, a[u]);
      }
  };
  // The next batch's loads are issued unconditionally: past the slice they fall outside the
  // buffer resources' range, return 0 and touch no memory.  A conditional prefetch made hipcc
  // wait vmcnt(0) where the two paths join -- for the prefetch itself and, as loads and stores
  // share vmcnt, for every store of the batch before: the double buffer then never overlapped
  // (tools/mix_probe.hip "persist2"; profiles/r4_vmcnt.txt).  A slice is at most kMaxSlice, so
  // the past-the-end offsets stay below 2^32.
  uint32_t b = 0;
  load(xa, aa, b);
  for (;;) {
    load(xb, ab, b + step);
    fold_store(xa, aa, b);
    if ((b += step) >= nvec) break;
    load(xa, aa, b + step);
    fold_store(xb, ab, b);
    if ((b += step) >= nvec) break;
  }
}

// Returns the leading bytes of the slice whose result it also pushed to the peers (PUSH = false:
// nothing is pushed and the value means nothing).
template <typename T, int OPC, bool VEC, bool PUSH = true>
__device__ __forceinline__ uint32_t read_fold(const CollParams& p, uint64_t coff, uint32_t nbytes, int lane) {
  if (!VEC) {
    read_fold_scalar<T, OPC>(p, coff, nbytes, lane, 0);
    return 0;
  }
  const int n = p.n, r = p.rank;
  const uint32_t nvec = nbytes >> 4;
  // (n >= 2 holds for every launched call, Comm::collective; stated, it keeps a rank count the
  // ladder below has no slot for out of it, and the compiler schedules the fold with that)
  if (n >= 2 && n <= 8) {
    // (2-byte types widen to f32 in reduce16: fewer vectors per peer keep the bf16 / fp16
    // variants within 256 registers without spilling)
    constexpr int h = sizeof(T) == 2 ? 1 : 0;
    if (!nvec) {
    } else if (n == 2) read_fold_all<T, OPC, 1, 12 - 4 * h, PUSH>(p, coff, nvec, lane);
    else if (n == 3) read_fold_all<T, OPC, 2, 8 - 2 * h, PUSH>(p, coff, nvec, lane);
    else if (n <= 5) read_fold_all<T, OPC, 4, 4 - h, PUSH>(p, coff, nvec, lane);
    else read_fold_all<T, OPC, 7, 3 - h, PUSH>(p, coff, nvec, lane);
    if (nbytes & 15u) read_fold_scalar<T, OPC>(p, coff, nbytes, lane, nvec * 16);
    return nvec * 16;
  }
  // (kPreMulSum on int32: half the batch -- with 16 vectors per stream the 32-bit multiplies spilled
  // 36 registers to scratch at the 256-register bound)
  constexpr int U = OPC == kPreMulSum && std::is_same<T, int32_t>::value ? kReadFoldU / 2 : kReadFoldU;
  const rsrc_t out = make_rsrc(p.recv + coff, nbytes);
  const char* lsrc = p.send + coff;
  uint32_t b = 0;
  // full batches: the n-1 remote streams are issued back to back (one peer ahead of the fold)
  for (; b + 64 * U <= nvec; b += 64 * U) {
    v4u acc[U], cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = ld_g16(lsrc + (size_t)(b + (uint32_t)(u * 64 + lane)) * 16);
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = prescale16<T, OPC>(acc[u], p.scale);
    {
      const rsrc_t in = make_rsrc(p.peer_send[direct_peer(n, r, 1)] + coff, nbytes);
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = ld_slot16(in, (b + (uint32_t)(u * 64 + lane)) * 16);
    }
    for (int k = 1; k < n; ++k) {
      if (k + 1 < n) {
        const rsrc_t in = make_rsrc(p.peer_send[direct_peer(n, r, k + 1)] + coff, nbytes);
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = ld_slot16(in, (b + (uint32_t)(u * 64 + lane)) * 16);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u] = reduce16<T, OPC>(prescale16<T, OPC>(cur[u], p.scale), acc[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) st_slot16(out, (b + (uint32_t)(u * 64 + lane)) * 16, acc[u]);
  }
  if (b < nvec) read_fold_wide<T, OPC>(p, coff, b, nvec, lane);
  if (nbytes & 15u) read_fold_scalar<T, OPC>(p, coff, nbytes, lane, nvec * 16);
  return 0;
}

// The folds that do not push as they fold (scalar, past 8 ranks): bytes [off0, nbytes) of my result
// slice, read back from my recv (stored and drained) into every peer's recv
template <typename T, bool VEC>
__device__ __forceinline__ void read_push_rest(const CollParams& p, uint64_t coff, uint32_t nbytes, uint32_t off0,
                                               int lane) {
  const int n = p.n, r = p.rank;
  const rsrc_t src = make_rsrc(p.recv + coff, nbytes);
  // 16-byte vectors only where the buffers are dword-aligned (VEC), element by element otherwise
  const uint32_t v0 = VEC ? (off0 + 15u) >> 4 : 0, v1 = VEC ? nbytes >> 4 : 0;
  for (int k = 1; k < n; ++k) {
    const rsrc_t dst = make_rsrc(p.peer_recv[direct_peer(n, r, k)] + coff, nbytes);
    for (uint32_t i = v0 + (uint32_t)lane; i < v1; i += 64) st_slot16(dst, i * 16, ld_slot16(src, i * 16));
    const uint32_t e0 = (v1 > v0 ? v1 * 16 : off0) / sizeof(T), ne = nbytes / sizeof(T);
    for (uint32_t i = e0 + (uint32_t)lane; i < ne; i += 64)
      Scal<sizeof(T)>::st(dst, i * (uint32_t)sizeof(T), Scal<sizeof(T)>::ld(src, i * (uint32_t)sizeof(T)));
  }
}

// Messages per (pair, pipeline) and call: START (my send is readable and my recv writable: the
// call began on my stream), DONE (I no longer read your buffers, my pushes into your recv have
// landed: your stream may go on).  Per pipeline: START, F0 F1 ... F(I-1), DONE.  The READY word
// counts iters + 2 messages per call (it jumps from START to DONE: the count the 4.0-5.x load
// form's per-iteration READYs kept, which the scratch schedules' slot counters still follow);
// DONE also returns credits for every message (the counters continue across calls, whatever the
// schedule).
template <typename T, int OPC, bool VEC>
__device__ __forceinline__ void read_body(const CollParams& p) {
  signal_start(p);
  const WaveId id = wave_id();
  // C: the communicator's pipelines (mailbox and counter layout); A: the ones this call runs
  // (its grid), slice s on pipeline s mod A
  const int lane = id.lane, w = id.w, C = p.pipes, A = id.C, wv = id.wv;
  const int n = p.n, r = p.rank;
  copy_tail(p, w, lane);
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  u64* tx = s_tx[wv];
  u64* rx = s_rx[wv];
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  const uint32_t iters = p.iters;
  const u64 mpc = read_msgs_per_call(iters);
  uint32_t seen = 0;  // a cause this wave saw itself (starts_agree), for its ABORT word
  if (lane < n) {
    tx[lane] = p.tx_seq[(u64)lane * C + w];
    rx[lane] = p.rx_seq[(u64)lane * C + w];
  }
  __builtin_amdgcn_wave_barrier();
  // START to every peer (with the call's signature on a registered-window call), then wait for theirs
  if (lane < n && lane != r) {
    if (p.sig) st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w) + kSigWord, p.sig);
    st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), tx[lane] + 1);
  }
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, w), rx[lane < n ? lane : 0] + 1, lane < n && lane != r, ctl, lane,
                       true))
    goto aborted;
  if (!starts_agree(p, ctl, C, lane, w, &seen)) goto aborted;
  acquire_sys(p.sys_fence);
  for (uint32_t j = 0; j < iters; ++j) {
    // F(j): fold my chunk's slice j from the peers' send buffers, store it and push it into every
    // peer's recv; no READY (the peers wait only for DONE, which drains every push), so no drain
    // per slice -- except before the part read back from my recv to be pushed
    const u64 s = (u64)j * A + w;
    const uint32_t len = (uint32_t)slice_len(p.chunk_bytes, p.slice_bytes, s);
    const u64 coff = (u64)r * p.chunk_bytes + s * p.slice_bytes;
    const uint32_t pushed = len ? read_fold<T, OPC, VEC>(p, coff, len, lane) : 0;
    if (pushed < len) {
      drain_stores();
      read_push_rest<T, VEC>(p, coff, len, pushed, lane);
    }
  }
  // DONE: every load of a peer's buffer has returned (and every push into the peers' recv has
  // landed); then wait until nobody reads mine (and every peer's pushes into mine have landed)
  drain_stores();
  if (p.sys_fence && lane == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (lane < n && lane != r) {
    st_sys(p.peer_mbox[lane] + mbox_credit(n, C, r, w), rx[lane] + mpc);
    st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), tx[lane] + mpc);
  }
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, w), rx[lane < n ? lane : 0] + mpc, lane < n && lane != r, ctl, lane,
                       false))
    goto aborted;
  if (lane < n && lane != r) {
    p.tx_seq[(u64)lane * C + w] = tx[lane] + mpc;
    p.rx_seq[(u64)lane * C + w] = rx[lane] + mpc;
  }
  return;
aborted:
  if (lane == 0)
    for (int k = 1; k < n; ++k) st_sys(p.peer_mbox[direct_peer(n, r, k)] + mbox_abort(n, C), abort_word(p, seen));
}

template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) read_kernel(CollParams p) {
  read_body<T, OPC, VEC>(p);
}
template <typename T, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scaled_read(CollParams p) {
  read_body<T, kPreMulSum, VEC>(p);
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) fp8_read(CollParams p) {
  read_body<T, OPC, VEC>(p);
}

// ---------------------------------------------------------------- the read schedule's two halves
// ncclReduceScatter (scatter_fold) and ncclAllGather (gather_push) on device buffers every rank
// can share: read_kernel's fold without its pushes, and its pushes without a fold.  Both run
// read_kernel's protocol message for message -- one pipeline per wave; START to every peer, wait
// for theirs, the slices, drain, DONE with the credits, wait for theirs; the counters advance by
// read_msgs_per_call(iters) -- so calls of any collective and schedule follow each other on one
// communicator, and a give-up ends as there (bounded waits, the peers' ABORT words).  Negotiated
// calls only (no registered windows): no signature to compare.  read_kernel keeps its own copy of
// the protocol: its fold sits at the 256-register bound and must compile to what it was.
// body(coff, len, lane): the slice at byte coff = r * chunk_bytes + s * slice_bytes, len bytes long.
// ROOTED (root_fold / root_relay): the chunks are ceil(count / n) elements, so each slice's length
// is additionally clamped to the buffer's end (schedule.h rooted_len).
// VAR (vhalf_fold / vhalf_push, per-rank counts): the call's geometry is the LARGEST block's, this
// rank's slices start at byte vbase of the array-side buffers and their lengths are clamped to its own
// block of vbytes (schedule.h vhalf_len) -- only the body is skipped once the block has run out, START
// and DONE are exchanged all the same.  Nothing of the protocol below depends on the block, nor on the
// body's VEC: it counts messages by p.iters alone, so ranks of one call may run different paths.
template <bool ROOTED = false, bool VAR = false, typename Body>
__device__ __forceinline__ void read_half(const CollParams& p, u64 (*s_tx)[kMaxRanks], u64 (*s_rx)[kMaxRanks],
                                          const Body& body, u64 vbase = 0, u64 vbytes = 0) {
  signal_start(p);
  const WaveId id = wave_id();
  const int lane = id.lane, w = id.w, C = p.pipes, A = id.C;
  const int n = p.n, r = p.rank;
  u64* tx = s_tx[id.wv];
  u64* rx = s_rx[id.wv];
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  const uint32_t iters = p.iters;
  const u64 mpc = read_msgs_per_call(iters);
  if (lane < n) {
    tx[lane] = p.tx_seq[(u64)lane * C + w];
    rx[lane] = p.rx_seq[(u64)lane * C + w];
  }
  __builtin_amdgcn_wave_barrier();
  // START: my send is readable and my recv writable (the call began on my stream); lane q speaks
  // for peer q.  (Control flow and expressions as in read_kernel: a shared `peer` flag and an `ok`
  // result carried over the slices cost the float fold 8 spilled registers at the 256 bound.)
  if (lane < n && lane != r) st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), tx[lane] + 1);
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, w), rx[lane < n ? lane : 0] + 1, lane < n && lane != r, ctl, lane,
                       true))
    goto aborted;
  acquire_sys(p.sys_fence);
  for (uint32_t j = 0; j < iters; ++j) {
    const u64 s = (u64)j * A + w;
    const uint32_t len = VAR      ? (uint32_t)vhalf_len(vbytes, p.slice_bytes, s)
                         : ROOTED ? (uint32_t)rooted_len(p.total_bytes, (u64)r * p.chunk_bytes, p.chunk_bytes, p.slice_bytes, s)
                                  : (uint32_t)slice_len(p.chunk_bytes, p.slice_bytes, s);
    const u64 coff = VAR ? vbase + s * p.slice_bytes : (u64)r * p.chunk_bytes + s * p.slice_bytes;
    if (len) body(coff, len, lane);
  }
  // DONE: every load of a peer's send has returned and every push into a peer's recv has landed
  drain_stores();
  if (p.sys_fence && lane == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (lane < n && lane != r) {
    st_sys(p.peer_mbox[lane] + mbox_credit(n, C, r, w), rx[lane] + mpc);
    st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), tx[lane] + mpc);
  }
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, w), rx[lane < n ? lane : 0] + mpc, lane < n && lane != r, ctl, lane,
                       false))
    goto aborted;
  if (lane < n && lane != r) {
    p.tx_seq[(u64)lane * C + w] = tx[lane] + mpc;
    p.rx_seq[(u64)lane * C + w] = rx[lane] + mpc;
  }
  return;
aborted:
  if (lane == 0)
    for (int k = 1; k < n; ++k) st_sys(p.peer_mbox[direct_peer(n, r, k)] + mbox_abort(n, C), abort_word(p));
}

// Reduce-scatter: rank r folds slice s of chunk r from every rank's send in ring order (the
// all-reduce's bits for that chunk) and stores it at the same slice offset of its recv -- p.recv is
// recv - r * chunk_bytes (Comm::launch), so the fold helpers address both with one offset; the
// shifted pointer is never dereferenced below recv.  Each GPU's HBM moves n + 1 chunks per call.
// In place (recv == send + r * chunk_bytes): only rank r reads chunk r of anyone's send, and it
// stores a batch after that batch's loads.
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scatter_fold(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); });
}
template <typename T, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scaled_scatter(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, kPreMulSum, VEC, false>(p, coff, len, lane); });
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) fp8_scatter(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); });
}

// ---------------------------------------------------------------- copy and push
// The loop of the all-gather (gather_push) and of the broadcast (root_relay): a slice of chunk r is
// loaded once from `from` and stored into this rank's recv and into the recv of D other ranks.
// Destination j of D, in ring order from r + 1, one rank left out (the broadcast's root in place):
__device__ __forceinline__ int push_peer(int n, int r, int j, int skip) {  // skip: ring distance to that rank, 0 = none
  const int k = 1 + j;
  return direct_peer(n, r, skip && k >= skip ? k + 1 : k);
}

// 16-byte vectors of one slice: V vectors per lane per batch, loaded non-temporal when `from` is
// this rank's own memory (LOCAL) and sc0 sc1 over the link otherwise, as the fold loads its peers;
// stored into this rank's recv and pushed into the D destinations' recv with the sc0 sc1 stores
// whose visibility to the owner's later kernels the all-reduce's pushes rely on (file header).
// Two batches in flight per wave: the next batch's loads leave before this one is stored --
// unconditionally, for the vmcnt reason read_fold_all explains; past the slice they fall outside
// the buffer resource, return 0 and touch nothing.  Pipeline w starts its pushes at destination
// w mod D, so a rank's pipelines spread over all links.  own = false (the chunk already is in this
// rank's recv): the own store's resource is empty and drops it.  G descriptor slots up to 8 ranks
// (they stay in SGPRs; a slot past D is empty); G = 0: any rank count, the destinations in a loop.
constexpr int kGatherV = 8;

template <int G, int V, bool LOCAL>
__device__ __forceinline__ void copy_push_vec(const CollParams& p, const char* from, uint64_t coff, uint32_t nvec, int lane,
                                              bool own, int D, int skip) {
  constexpr uint32_t step = 64 * V;
  constexpr int GS = G > 0 ? G : 1;
  const int n = p.n, r = p.rank, w = wave_id().w;
  const uint32_t vb = nvec * 16;
  const rsrc_t src = make_rsrc(from + coff, vb), out = make_rsrc(p.recv + coff, own ? vb : 0u);
  rsrc_t pout[GS];
#pragma unroll
  for (int g = 0; g < G; ++g) pout[g] = make_rsrc(p.peer_recv[push_peer(n, r, g < D ? (g + w) % D : 0, skip)] + coff, g < D ? vb : 0u);
  v4u xa[V], xb[V];
  auto load = [&](v4u(&x)[V], uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u)
      x[u] = LOCAL ? ld_nt16(src, (b + (uint32_t)(u * 64 + lane)) * 16) : ld_slot16(src, (b + (uint32_t)(u * 64 + lane)) * 16);
  };
  auto store = [&](v4u(&x)[V], uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) st_slot16(out, (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
    if (G > 0) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (g < D) {
#pragma unroll
          for (int u = 0; u < V; ++u) st_slot16(pout[g], (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
        }
    } else {
      for (int j = 0; j < D; ++j) {
        const rsrc_t po = make_rsrc(p.peer_recv[push_peer(n, r, (j + w) % D, skip)] + coff, vb);
#pragma unroll
        for (int u = 0; u < V; ++u) st_slot16(po, (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
      }
    }
  };
  uint32_t b = 0;
  load(xa, b);
  for (;;) {
    load(xb, b + step);
    store(xa, b);
    if ((b += step) >= nvec) break;
    load(xa, b + step);
    store(xb, b);
    if ((b += step) >= nvec) break;
  }
}

// slice `nbytes` at byte `coff` of `from` into the same offset of every recv; the last nbytes % 16
// bytes, and everything without VEC, element by element
template <int ESZ, bool VEC, bool LOCAL>
__device__ __forceinline__ void copy_push_slice(const CollParams& p, const char* from, bool own, int D, int skip,
                                                uint64_t coff, uint32_t nbytes, int lane) {
  const int n = p.n, r = p.rank;
  uint32_t done = 0;
  if (VEC) {
    const uint32_t nvec = nbytes >> 4;
    if (!nvec) {
    } else if (n == 2) copy_push_vec<1, kGatherV, LOCAL>(p, from, coff, nvec, lane, own, D, skip);
    else if (n == 3) copy_push_vec<2, kGatherV, LOCAL>(p, from, coff, nvec, lane, own, D, skip);
    else if (n <= 5) copy_push_vec<4, kGatherV, LOCAL>(p, from, coff, nvec, lane, own, D, skip);
    else if (n <= 8) copy_push_vec<7, kGatherV, LOCAL>(p, from, coff, nvec, lane, own, D, skip);
    else copy_push_vec<0, kGatherV, LOCAL>(p, from, coff, nvec, lane, own, D, skip);
    done = nvec * 16;
  }
  if (done == nbytes) return;
  typedef Scal<ESZ> S;
  const rsrc_t src = make_rsrc(from + coff, nbytes), out = make_rsrc(p.recv + coff, own ? nbytes : 0u);
  const uint32_t ne = nbytes / ESZ;
  for (uint32_t i = done / ESZ + (uint32_t)lane; i < ne; i += 64) {
    const typename S::U v = S::ld(src, i * (uint32_t)ESZ);
    S::st(out, i * (uint32_t)ESZ, v);
    for (int j = 0; j < D; ++j) S::st(make_rsrc(p.peer_recv[push_peer(n, r, j, skip)] + coff, nbytes), i * (uint32_t)ESZ, v);
  }
}

// All-gather: the slice comes from the same offset of p.send (send - r * chunk_bytes, Comm::launch)
// and goes to all n - 1 peers; in place, this rank's chunk already is in its recv.  No arithmetic,
// so by element size only.  Only rank q ever writes chunk q of any recv, and nobody reads a recv
// inside the call.  Each GPU's HBM moves n + 1 chunks per call (one read, n writes landing in it).
// (The kernels that only copy have their code in a *_body function too: the entry point named for
// the element sizes 2 / 4 / 8, and a `byte_*` one for element size 1 -- the fp8 types -- beside it.)
template <int ESZ, bool VEC>
__device__ __forceinline__ void gather_body(const CollParams& p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) {
    copy_push_slice<ESZ, VEC, true>(p, p.send, p.send != p.recv, p.n - 1, 0, coff, len, lane);
  });
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) gather_push(CollParams p) {
  gather_body<ESZ, VEC>(p);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_gather(CollParams p) {
  gather_body<1, VEC>(p);
}

// ---------------------------------------------------------------- the halves with per-rank counts
// mncclReduceScatterv (vhalf_fold) and mncclAllGatherv (vhalf_push) on device buffers every rank can
// share: scatter_fold and gather_push with a per-rank base and length (kernels.h VHalfArgs, a second
// by-value argument), in read_half<VAR>'s protocol message for message.  The arrays are the same on
// every rank, so one byte offset serves every rank's array-side buffer: rank r's block sits at byte
// v.base of every send (the fold) / of every recv (the push).  The geometry is the largest block's
// (p.chunk_bytes = M on every rank); a rank whose block is short or empty runs fewer or no bodies
// and the same START and DONE.
// Fold: rank r folds its block out of every rank's send at v.base, in the all-reduce's order for
// chunk r (read_fold<.., PUSH = false>), into its recv -- p.recv is recv - v.base (Comm::vhalf), as
// scatter_fold's is recv - r * chunk_bytes, and is never dereferenced below recv.  In place (recv ==
// send + v.base): only rank r reads block r of anyone's send, and it stores a batch after that
// batch's loads; the blocks do not overlap (vhalves.h), so no peer reads what it writes.
// Push: each slice of send is loaded ONCE (p.send is send - v.base) and stored at v.base of this
// rank's recv and of every peer's (copy_push_slice); in place, the own store is dropped.
// (The one-byte entry points are vhalf_fp8 / vhalf_byte, not fp8_* / byte_* like the other families':
// every name of this family starts with what it belongs to.)
// VEC is this rank's alone (vhalves.h vhalf_vec): a rank whose base or length is odd takes the
// element path while its peers take vectors -- see read_half: the protocol does not see it.
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) vhalf_fold(CollParams p, VHalfArgs v) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<false, true>(
      p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); },
      v.base, v.bytes);
}
template <typename T, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scaled_vhalf(CollParams p, VHalfArgs v) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<false, true>(
      p, s_tx, s_rx,
      [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, kPreMulSum, VEC, false>(p, coff, len, lane); }, v.base,
      v.bytes);
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) vhalf_fp8(CollParams p, VHalfArgs v) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<false, true>(
      p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); },
      v.base, v.bytes);
}
template <int ESZ, bool VEC>
__device__ __forceinline__ void vhalf_push_body(const CollParams& p, const VHalfArgs& v) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<false, true>(
      p, s_tx, s_rx,
      [&p](u64 coff, uint32_t len, int lane) {
        copy_push_slice<ESZ, VEC, true>(p, p.send, p.send != p.recv, p.n - 1, 0, coff, len, lane);
      },
      v.base, v.bytes);
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) vhalf_push(CollParams p, VHalfArgs v) {
  vhalf_push_body<ESZ, VEC>(p, v);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) vhalf_byte(CollParams p, VHalfArgs v) {
  vhalf_push_body<1, VEC>(p, v);
}

// ---------------------------------------------------------------- the rooted collectives
// ncclReduce (root_fold) and ncclBroadcast (root_relay) on device buffers every rank can share,
// in read_half's protocol message for message.  Neither lets the root do the work: a root that
// folded or pushed everything itself would move the whole buffer B over each of its links while
// every other link idled.  Here every rank works on chunk `rank` (ceil(count / n) elements, the
// trailing chunks short or empty), so each link into the root carries about 2B/n (derived from the
// schedule, not measured: no run with ranks on distinct GPUs exists).
//
// Reduce: rank r folds its slices of chunk r from all n send buffers -- read_fold's fold, order,
// batching and unconditional prefetch -- and stores the result at the same offset of the ROOT's
// recv: p.recv is the root's recv on every rank (Comm::launch passes this rank's mapping of it), so
// the fold helpers address it as scatter_fold's do.  On every rank but the root that store is a
// push into another agent's memory and needs the all-reduce's push-visibility guarantee (file
// header): sc0 sc1, as every store of the fold is.  A non-root rank writes nothing to a buffer
// of its own.  In place on the root (recv == send): the reduce-scatter's argument -- only rank c
// reads chunk c of anyone's send, and it stores a batch after that batch's loads.  Each GPU's HBM
// serves n chunk reads, the root's also takes n chunk writes; a link into the root carries the
// root's loads of chunk `root` and rank r's pushed chunk (derived).
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) root_fold(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<true>(p, s_tx, s_rx,
                  [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); });
}
template <typename T, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) scaled_root(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<true>(p, s_tx, s_rx,
                  [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, kPreMulSum, VEC, false>(p, coff, len, lane); });
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) fp8_root(CollParams p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half<true>(p, s_tx, s_rx,
                  [&p](u64 coff, uint32_t len, int lane) { (void)read_fold<T, OPC, VEC, false>(p, coff, len, lane); });
}

// Broadcast: rank r copies its slices of chunk r from the root's send -- sc0 sc1 loads over the
// link, as the fold loads its peers; the root reads its own send non-temporal, as gather_push does
// (ROOT) -- into its own recv and into the recv of every other rank: the all-gather's loop
// (copy_push_slice) with another source and destination set.  The root's recv is a destination like any other when the
// root's call is out of place (so the root's own copy happens inside the kernel, chunk by chunk,
// by the rank that loaded the chunk anyway) and is left out when it is in place: every rank sees
// that from its mappings, peer_send[root] == peer_recv[root] (were the test ever wrong, the push
// would store the bytes just loaded from that address: only rank c touches chunk c).  So a
// non-root rank pushes into n - 2 peers (n - 1 with the root's recv), the root into n - 1; at
// n = 2 there is no relay.  The root's links carry 2B/n each, the others B/n (derived).
//
// No arithmetic, so by element size only.  Only rank c ever writes chunk c of any recv, nobody
// reads a recv inside the call, and the root's send is only read (in place: see above).
template <int ESZ, bool VEC>
__device__ __forceinline__ void relay_body(const CollParams& p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  // one slice, by role: its source, whether this rank's recv takes it, and the D destinations
  auto slice = [&p](auto is_root, u64 coff, uint32_t len, int lane) {
    constexpr bool ROOT = decltype(is_root)::value;
    const int n = p.n, r = p.rank, root = p.root;
    const bool root_in_place = p.peer_send[root] == p.peer_recv[root];
    const bool own = !(ROOT && root_in_place);  // the root in place: its chunk already is in its recv
    const int skip = !ROOT && root_in_place ? mod_n(root - r, n) : 0;
    const int D = n - 1 - (skip ? 1 : 0);
    copy_push_slice<ESZ, VEC, ROOT>(p, ROOT ? p.send : p.peer_send[root], own, D, skip, coff, len, lane);
  };
  if (p.rank == p.root)
    read_half<true>(p, s_tx, s_rx, [&](u64 coff, uint32_t len, int lane) { slice(std::true_type{}, coff, len, lane); });
  else
    read_half<true>(p, s_tx, s_rx, [&](u64 coff, uint32_t len, int lane) { slice(std::false_type{}, coff, len, lane); });
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) root_relay(CollParams p) {
  relay_body<ESZ, VEC>(p);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_relay(CollParams p) {
  relay_body<1, VEC>(p);
}

// ---------------------------------------------------------------- the all-to-all
// ncclAllToAll (exchange_push) on device buffers every rank can share, in read_half's protocol
// message for message: block q of rank r's send becomes block r of rank q's recv; a chunk is one
// block, and both buffers hold n of them.  For slice s of the call, pipeline w of rank r loads the
// slice of EVERY block q from its own send, non-temporal as gather_push reads its send, and pushes
// it into rank q's recv at block r -- its own block into its own recv.  Every off-diagonal block
// crosses exactly one link exactly once, and all n - 1 links of a rank are busy for the whole call.
//
// It pushes rather than pulls: the all-gather and the all-reduce already rest on pushed sc0 sc1
// stores being visible to the owner's later kernels (file header).  A pull form -- rank q loading
// block q of every peer's send -- would rest on a second cross-device property, a peer's earlier
// plain stores into its send being visible to loads over the link, that nobody has observed for
// this pattern.  Only rank r ever writes block r of any recv, nobody reads a recv inside the call,
// and the buffers of a call never overlap (Comm::collective refuses it): there is no in-place form.
// Each GPU's HBM moves 2n blocks per call (n read, n landing); each link carries one block each way.
//
// 16-byte vectors of one slice, V per lane per batch.  The (destination, batch) pairs of the slice
// form one sequence -- destination by destination, the peers in direct_peer order starting at peer
// w mod n-1 so a rank's pipelines spread over all links, this rank itself last -- and two of its
// batches are in flight per wave: the next batch's loads leave before this one is stored, across
// destinations too, unconditionally (the vmcnt reason read_fold_all explains).  Past the slice the
// loads fall outside the buffer resource, return 0 and touch nothing; past the last destination the
// resource is empty.  The descriptors are rebuilt from the kernel's arguments when the destination
// changes (wave-uniform: they stay in SGPRs), so one form serves every rank count.
constexpr int kExchangeV = 8;

template <int V>
__device__ __forceinline__ void exchange_push_vec(const CollParams& p, uint64_t soff, uint32_t nvec, int lane) {
  constexpr uint32_t step = 64 * V;
  const int n = p.n, r = p.rank, first = wave_id().w % (n - 1);
  const uint32_t vb = nvec * 16;
  const u64 cb = p.chunk_bytes, mine = (u64)r * cb + soff;
  // destination k of n (k == n: past the end, nothing is loaded)
  auto dest = [&](int k) { return k < n - 1 ? direct_peer(n, r, 1 + (first + k) % (n - 1)) : r; };
  auto src_of = [&](int k) { return make_rsrc(p.send + (u64)dest(k) * cb + soff, k < n ? vb : 0u); };
  auto dst_of = [&](int k) { return make_rsrc((k < n - 1 ? const_cast<char*>(p.peer_recv[dest(k)]) : p.recv) + mine, vb); };
  auto load = [&](v4u(&x)[V], rsrc_t s, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) x[u] = ld_nt16(s, (b + (uint32_t)(u * 64 + lane)) * 16);
  };
  auto store = [&](v4u(&x)[V], rsrc_t d, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) st_slot16(d, (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
  };
  int k = 0;       // the batch about to be stored: destination k, vectors from b
  uint32_t b = 0;
  rsrc_t src = src_of(0), dst = dst_of(0);
  v4u xa[V], xb[V];
  // loads the batch after (k, b) into nxt, stores cur, moves on; false after the last batch
  auto turn = [&](v4u(&cur)[V], v4u(&nxt)[V]) {
    int k2 = k;
    uint32_t b2 = b + step;
    if (b2 >= nvec) {
      b2 = 0;
      src = src_of(++k2);
    }
    load(nxt, src, b2);
    store(cur, dst, b);
    if (k2 != k) dst = dst_of(k2);
    k = k2;
    b = b2;
    return k < n;
  };
  load(xa, src, 0);
  while (turn(xa, xb) && turn(xb, xa)) {
  }
}

// slice `nbytes` at byte `soff` of every block; the last nbytes % 16 bytes, and everything without
// VEC, element by element
template <int ESZ, bool VEC>
__device__ __forceinline__ void exchange_slice(const CollParams& p, uint64_t soff, uint32_t nbytes, int lane) {
  const int n = p.n, r = p.rank;
  uint32_t done = 0;
  if (VEC) {
    const uint32_t nvec = nbytes >> 4;
    if (nvec) exchange_push_vec<kExchangeV>(p, soff, nvec, lane);
    done = nvec * 16;
  }
  if (done == nbytes) return;
  typedef Scal<ESZ> S;
  const uint32_t ne = nbytes / ESZ;
  const u64 cb = p.chunk_bytes, mine = (u64)r * cb + soff;
  for (int k = 1; k <= n; ++k) {
    const int q = direct_peer(n, r, k);  // k == n: this rank itself
    const rsrc_t src = make_rsrc(p.send + (u64)q * cb + soff, nbytes);
    const rsrc_t dst = make_rsrc((q == r ? p.recv : const_cast<char*>(p.peer_recv[q])) + mine, nbytes);
    for (uint32_t i = done / ESZ + (uint32_t)lane; i < ne; i += 64) S::st(dst, i * (uint32_t)ESZ, S::ld(src, i * (uint32_t)ESZ));
  }
}

// No arithmetic, so by element size only.  read_half hands the slice's offset in chunk `rank`; the
// slice's offset within a block is what every block shares.
template <int ESZ, bool VEC>
__device__ __forceinline__ void exchange_body(const CollParams& p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) {
    exchange_slice<ESZ, VEC>(p, coff - (u64)p.rank * p.chunk_bytes, len, lane);
  });
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) exchange_push(CollParams p) {
  exchange_body<ESZ, VEC>(p);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_exchange(CollParams p) {
  exchange_body<1, VEC>(p);
}

// ---------------------------------------------------------------- gather and scatter
// ncclGather (collect_push) and ncclScatter (deal_push) on device buffers every rank can share, in
// read_half's protocol message for message: column `root` and row `root` of the all-to-all.  A chunk
// is one block; the root's large buffer holds n of them.
//   Gather: pipeline w of rank r loads slice s of its one block from its own send (p.send is
//   send - r * chunk_bytes, Comm::make_params, as for the all-gather) and pushes it into block r of
//   the ROOT's recv; the root stores its own block into its own recv unless the call is in place
//   (p.send == p.recv then).  A non-root writes nothing of its own, and all of its pipelines drive
//   its one link to the root.
//   Scatter: the root's pipeline w loads slice s of EVERY block q from its send and pushes it into
//   rank q's recv -- the destination side gets NO block offset: peer_recv[q] is rank q's recv itself
//   -- its own block into its own recv (p.recv is recv - r * chunk_bytes, as for the
//   reduce-scatter; in place p.recv == p.send) unless the call is in place.  The destinations run
//   in direct_peer order from peer w mod n-1, this rank itself last, so the root's pipelines spread
//   over all its links.  The other ranks run START ("my recv is writable") and DONE (whose wait
//   means "my block has landed") only.
// Pushes, not pulls, for exchange_push's reason; each link into or out of the root carries exactly
// one block, so relaying through other ranks would gain nothing.  Only rank r ever writes block r
// of the root's recv (gather); only the root writes any recv (scatter); nobody reads a recv inside
// the call.  n blocks move through the root's HBM, one through every other rank's (derived from the
// schedule, not measured: no run with ranks on distinct GPUs exists).
//
// 16-byte vectors of one slice, exchange_push_vec's loop over K (source, destination) pairs the
// caller describes: V vectors per lane per batch, two batches in flight per wave -- the next
// batch's loads leave before this one is stored, across pairs too, unconditionally (the vmcnt
// reason read_fold_all explains).  Past the slice the loads fall outside the buffer resource,
// return 0 and touch nothing; src_of(k) and dst_of(k) for k >= K must be empty resources.  K >= 1.
constexpr int kDealV = 8;

template <int V, typename Src, typename Dst>
__device__ __forceinline__ void push_pairs_vec(int K, const Src& src_of, const Dst& dst_of, uint32_t nvec, int lane) {
  constexpr uint32_t step = 64 * V;
  auto load = [&](v4u(&x)[V], rsrc_t s, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) x[u] = ld_nt16(s, (b + (uint32_t)(u * 64 + lane)) * 16);
  };
  auto store = [&](v4u(&x)[V], rsrc_t d, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) st_slot16(d, (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
  };
  int k = 0;       // the batch about to be stored: pair k, vectors from b
  uint32_t b = 0;
  rsrc_t src = src_of(0), dst = dst_of(0);
  v4u xa[V], xb[V];
  // loads the batch after (k, b) into nxt, stores cur, moves on; false after the last batch
  auto turn = [&](v4u(&cur)[V], v4u(&nxt)[V]) {
    int k2 = k;
    uint32_t b2 = b + step;
    if (b2 >= nvec) {
      b2 = 0;
      src = src_of(++k2);
    }
    load(nxt, src, b2);
    store(cur, dst, b);
    if (k2 != k) dst = dst_of(k2);
    k = k2;
    b = b2;
    return k < K;
  };
  load(xa, src, 0);
  while (turn(xa, xb) && turn(xb, xa)) {
  }
}

// the same pairs' bytes [done, nbytes), element by element
template <int ESZ, typename Src, typename Dst>
__device__ __forceinline__ void push_pairs_scalar(int K, const Src& src_of, const Dst& dst_of, uint32_t done,
                                                  uint32_t nbytes, int lane) {
  typedef Scal<ESZ> S;
  const uint32_t ne = nbytes / ESZ;
  for (int k = 0; k < K; ++k) {
    const rsrc_t src = src_of(k), dst = dst_of(k);
    for (uint32_t i = done / ESZ + (uint32_t)lane; i < ne; i += 64) S::st(dst, i * (uint32_t)ESZ, S::ld(src, i * (uint32_t)ESZ));
  }
}

// Gather: slice `nbytes` at byte coff = r * chunk_bytes + s * slice_bytes of the root's recv
template <int ESZ, bool VEC>
__device__ __forceinline__ void collect_slice(const CollParams& p, uint64_t coff, uint32_t nbytes, int lane) {
  const bool is_root = p.rank == p.root;
  if (is_root && p.send == p.recv) return;  // the root in place: its block already is in its recv
  const char* from = p.send + coff;
  char* to = (is_root ? p.recv : const_cast<char*>(p.peer_recv[p.root])) + coff;
  uint32_t span = 0;  // the bytes the one pair's resources cover: the whole vectors, then the slice
  auto src_of = [&](int k) { return make_rsrc(from, k < 1 ? span : 0u); };
  auto dst_of = [&](int k) { return make_rsrc(to, k < 1 ? span : 0u); };
  const uint32_t vb = VEC ? nbytes & ~15u : 0u;
  span = vb;
  if (vb) push_pairs_vec<kDealV>(1, src_of, dst_of, vb >> 4, lane);
  if (vb == nbytes) return;
  span = nbytes;
  push_pairs_scalar<ESZ>(1, src_of, dst_of, vb, nbytes, lane);
}

// Scatter, on the root: slice `nbytes` at byte `soff` of every block
template <int ESZ, bool VEC>
__device__ __forceinline__ void deal_slice(const CollParams& p, uint64_t soff, uint32_t nbytes, int lane) {
  const int n = p.n, r = p.rank, first = wave_id().w % (n - 1);
  const u64 cb = p.chunk_bytes;
  const int K = n - 1 + (p.send != p.recv ? 1 : 0);  // in place: the root's block already is in its recv
  // pair k: the peers in direct_peer order from peer w mod n-1, then this rank itself
  auto dest = [&](int k) { return k < n - 1 ? direct_peer(n, r, 1 + (first + k) % (n - 1)) : r; };
  uint32_t span = 0;  // the bytes the pairs' resources cover: the whole vectors, then the slice
  auto src_of = [&](int k) { return make_rsrc(p.send + (u64)dest(k) * cb + soff, k < K ? span : 0u); };
  auto dst_of = [&](int k) {
    return make_rsrc(k < n - 1 ? const_cast<char*>(p.peer_recv[dest(k)]) + soff : p.recv + (u64)r * cb + soff,
                     k < K ? span : 0u);
  };
  const uint32_t vb = VEC ? nbytes & ~15u : 0u;
  span = vb;
  if (vb) push_pairs_vec<kDealV>(K, src_of, dst_of, vb >> 4, lane);
  if (vb == nbytes) return;
  span = nbytes;
  push_pairs_scalar<ESZ>(K, src_of, dst_of, vb, nbytes, lane);
}

// No arithmetic, so by element size only.  launch_persistent refuses a root outside [0, n).
template <int ESZ, bool VEC>
__device__ __forceinline__ void collect_body(const CollParams& p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) { collect_slice<ESZ, VEC>(p, coff, len, lane); });
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) collect_push(CollParams p) {
  collect_body<ESZ, VEC>(p);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_collect(CollParams p) {
  collect_body<1, VEC>(p);
}

// read_half hands the slice's offset in chunk `rank`; the slice's offset within a block is what
// every block shares.
template <int ESZ, bool VEC>
__device__ __forceinline__ void deal_body(const CollParams& p) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p](u64 coff, uint32_t len, int lane) {
    if (p.rank == p.root) deal_slice<ESZ, VEC>(p, coff - (u64)p.rank * p.chunk_bytes, len, lane);
  });
}
template <int ESZ, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) deal_push(CollParams p) {
  deal_body<ESZ, VEC>(p);
}
template <bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_deal(CollParams p) {
  deal_body<1, VEC>(p);
}

// ---------------------------------------------------------------- the variable all-to-all
// ncclAllToAllv (varblock_push) on device buffers every rank can share, in read_half's protocol
// message for message: the block this rank sends to rank q has its own length, its own offset in
// this rank's send and its own offset in rank q's recv (VarBlockArgs, the kernel's second argument:
// the host has every rank's row from the rendezvous).  The call's geometry is the all-to-all's for
// the LARGEST block of the whole matrix -- p.chunk_bytes, the same on every rank, so every pair's
// counters advance alike -- and slice s covers bytes [s * slice, s * slice + varblock_len) of every
// block: shorter blocks run out earlier, empty ones never start.  Pushes, not pulls, for
// exchange_push's reason; only rank r writes the block from r of any recv, and the blocks of a call
// overlap neither each other nor a send block (Comm::all_to_all_v refuses it).
//
// 16-byte vectors, exchange_push_vec's structure: the (destination, batch) pairs of the slice form
// one sequence -- the peers in direct_peer order from peer w mod n-1, this rank itself last, a
// destination with no vector in this slice skipped -- and the next batch's loads leave before this
// batch is stored, across destinations too.  Each destination has its own vector count, and its
// descriptors cover exactly its whole vectors: lanes past them read 0 and store nothing.  A
// destination takes this path when its source and destination addresses are both dword-aligned
// (v.vec_mask, wave-uniform); its last len % 16 bytes, and every other destination, go element by
// element as exchange_slice's scalar path does -- one odd bf16 displacement costs one destination
// the vectors, not the call.
template <int V>
__device__ __forceinline__ void varblock_push_vec(const CollParams& p, const VarBlockArgs& v, uint64_t soff, int lane) {
  constexpr uint32_t step = 64 * V;
  const int n = p.n, r = p.rank, first = wave_id().w % (n - 1);
  auto dest = [&](int k) { return k < n - 1 ? direct_peer(n, r, 1 + (first + k) % (n - 1)) : r; };
  // whole vectors of destination k in this slice (0: not a vector destination, exhausted, or k past the end)
  auto nvec_of = [&](int k) -> uint32_t {
    if (k >= n) return 0u;
    const int q = dest(k);
    return (v.vec_mask >> q) & 1u ? (uint32_t)(varblock_len_at(v.bytes[q], p.slice_bytes, soff) >> 4) : 0u;
  };
  auto next_from = [&](int k) {
    while (k < n && nvec_of(k) == 0) ++k;
    return k;
  };
  auto src_of = [&](int k, uint32_t nv) { return make_rsrc(p.send + (k < n ? v.src_off[dest(k)] : 0) + soff, nv * 16); };
  auto dst_of = [&](int k, uint32_t nv) {
    const int q = dest(k < n ? k : n - 1);
    return make_rsrc((q == r ? p.recv : const_cast<char*>(p.peer_recv[q])) + v.dst_off[q] + soff, nv * 16);
  };
  auto load = [&](v4u(&x)[V], rsrc_t s, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) x[u] = ld_nt16(s, (b + (uint32_t)(u * 64 + lane)) * 16);
  };
  auto store = [&](v4u(&x)[V], rsrc_t d, uint32_t b) {
#pragma unroll
    for (int u = 0; u < V; ++u) st_slot16(d, (b + (uint32_t)(u * 64 + lane)) * 16, x[u]);
  };
  int k = next_from(0);  // the batch about to be stored: destination k, vectors from b of its nvec
  if (k >= n) return;
  uint32_t b = 0, nvec = nvec_of(k);
  rsrc_t src = src_of(k, nvec), dst = dst_of(k, nvec);
  v4u xa[V], xb[V];
  // loads the batch after (k, b) into nxt, stores cur, moves on; false after the last batch
  auto turn = [&](v4u(&cur)[V], v4u(&nxt)[V]) {
    int k2 = k;
    uint32_t b2 = b + step, nvec2 = nvec;
    if (b2 >= nvec) {
      b2 = 0;
      k2 = next_from(k + 1);
      nvec2 = nvec_of(k2);
      src = src_of(k2, nvec2);  // past the last destination: empty, the loads return 0
    }
    load(nxt, src, b2);
    store(cur, dst, b);
    if (k2 != k) dst = dst_of(k2, nvec2);
    k = k2;
    b = b2;
    nvec = nvec2;
    return k < n;
  };
  load(xa, src, 0);
  while (turn(xa, xb) && turn(xb, xa)) {
  }
}

constexpr int kVarBlockV = 8;

// slice at byte `soff` of every block: the vector destinations' whole vectors first, then element by
// element each vector destination's last len % 16 bytes and every byte of the others
template <int ESZ>
__device__ __forceinline__ void varblock_slice(const CollParams& p, const VarBlockArgs& v, uint64_t soff, int lane) {
  const int n = p.n, r = p.rank;
  if (v.vec_mask) varblock_push_vec<kVarBlockV>(p, v, soff, lane);
  typedef Scal<ESZ> S;
  for (int k = 1; k <= n; ++k) {
    const int q = direct_peer(n, r, k);  // k == n: this rank itself
    const uint32_t len = (uint32_t)varblock_len_at(v.bytes[q], p.slice_bytes, soff);
    const uint32_t done = (v.vec_mask >> q) & 1u ? len & ~15u : 0u;
    if (done == len) continue;
    const rsrc_t src = make_rsrc(p.send + v.src_off[q] + soff, len);
    const rsrc_t dst = make_rsrc((q == r ? p.recv : const_cast<char*>(p.peer_recv[q])) + v.dst_off[q] + soff, len);
    const uint32_t ne = len / ESZ;
    for (uint32_t i = done / ESZ + (uint32_t)lane; i < ne; i += 64) S::st(dst, i * (uint32_t)ESZ, S::ld(src, i * (uint32_t)ESZ));
  }
}

// No arithmetic, so by element size only; the path is chosen per destination at run time.
// read_half hands the slice's offset in chunk `rank` of the largest-block geometry; the slice's
// offset within a block is what every block shares.
template <int ESZ>
__device__ __forceinline__ void varblock_body(const CollParams& p, const VarBlockArgs& v) {
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  read_half(p, s_tx, s_rx, [&p, &v](u64 coff, uint32_t, int lane) {
    varblock_slice<ESZ>(p, v, coff - (u64)p.rank * p.chunk_bytes, lane);
  });
}
template <int ESZ>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) varblock_push(CollParams p, VarBlockArgs v) {
  varblock_body<ESZ>(p, v);
}
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) byte_varblock(CollParams p, VarBlockArgs v) {
  varblock_body<1>(p, v);
}

// ---------------------------------------------------------------- point to point
// ncclSend / ncclRecv (p2p_kernel): a send is the sender's half of one ring hop to an arbitrary
// peer, a recv the receiver's half, on the scratch protocol of the file header -- the peer's region
// of the receiver's scratch (one per peer: schedule.h region_index), the pair's monotone READY /
// CREDIT words and its device-side counters, which continue across calls, schedules and graph
// replays.  No host rendezvous: two ranks exchange while the others do nothing.
//
// One launch runs a whole group (p2p.h P2pArgs, the second by-value argument).  Every directed pair
// present in the group -- the sends to one peer, or the recvs from one peer -- gets its OWN waves,
// one per pipeline, and a pair's waves run that pair's operations one after another; no wave ever
// serves two pairs.  (A wave that alternated a send slice and a recv slice would deadlock against a
// peer that receives and then sends ungrouped as soon as the message outgrows the slots.)  With at
// most 2 (n - 1) pairs x schedule.h p2p_pipes waves the launch stays inside the resident budget:
// all its waves are resident together.  A message's slices and pipelines follow from its byte count
// and the rank-uniform configuration alone (schedule.h p2p_msg_pipes), so both ends agree without
// talking.  Each end picks the 16-byte or the element path from ITS OWN pointer: the slot holds
// plain bytes at an aligned offset, so the two ends may differ; no arithmetic, so the element path
// moves 2-byte elements whatever the datatype (every supported size is a multiple).
//
// Sender, per slice: wait for the CREDIT of message seq - slots; load its own bytes and store them
// into the peer's slot (sc0 sc1: move<kSend>); drain; lane 0 publishes READY.  Receiver, per slice:
// poll READY; load the slot (sc0 sc1) and store into recv (move<kCopy>); drain; lane 0 returns the
// CREDIT.  Every spin is wait_ge_spin's: bounded, abort-aware, the first give-up claims the status
// and raises the peer's ABORT word.  A self pair is one copy by waves of their own.
typedef _Float16 P2pElem;  // the element path's 2-byte unit (moved, never used for arithmetic)

// a 64-bit value every lane holds alike, moved to scalar registers: the counter a wave loads from
// memory then keeps its slice loop, its waits and its slot descriptors wave-uniform
__device__ __forceinline__ u64 uniform64(u64 v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// The element path moves 2-byte units; a message of a one-byte datatype (the fp8 types) may end on an
// odd byte, which only a message's last slice can hold: lane 0 moves it, into the slot or out of it.
__device__ __forceinline__ void p2p_last_byte(bool sends, char* at, rsrc_t slot, uint32_t len, int lane) {
  if (!(len & 1u) || lane != 0) return;
  if (sends) Scal<1>::st(slot, len - 1, (uint8_t)at[len - 1]);
  else at[len - 1] = (char)Scal<1>::ld(slot, len - 1);
}

// the self copies, spread over the launch's self waves: wave k of K takes batches k, k + K, ...
__device__ __forceinline__ void p2p_self_copies(const P2pArgs& a, int k, int lane) {
  const int K = a.self_waves;
  for (int c = 0; c < a.nself; ++c) {
    const int i = a.self_first + 2 * c;
    const char* src = reinterpret_cast<const char*>(a.ptr[i]);
    char* dst = reinterpret_cast<char*>(a.ptr[i + 1]);
    const u64 bytes = a.bytes[i];
    const u64 nvec = a.vec[i] ? bytes >> 4 : 0;
    for (u64 v = (u64)k * 64 + (u64)lane; v < nvec; v += (u64)K * 64) st_g16(dst + v * 16, ld_g16(src + v * 16));
    if (k == 0)
      for (u64 b = nvec * 16 + (u64)lane; b < bytes; b += 64) dst[b] = src[b];
  }
}

__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) p2p_kernel(CollParams p, P2pArgs a) {
  signal_start(p);
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const int nwaves = a.npairs * a.pipes;
  if (b >= nwaves) {
    p2p_self_copies(a, b - nwaves, lane);
    return;
  }
  // C: the communicator's pipelines (mailbox, scratch and counter layout); w: this wave's pipeline
  const int pair = b / a.pipes, w = b % a.pipes, C = p.pipes;
  const int n = p.n, r = p.rank, K = p.nslots;
  const int peer = a.pair_peer[pair], first = a.pair_first[pair], count = a.pair_count[pair];
  const bool sends = a.pair_send[pair] != 0;
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  u64* ctr = (sends ? p.tx_seq : p.rx_seq) + (u64)peer * C + w;
  u64 seq = uniform64(*ctr);
  // the word this wave waits on (in this rank's mailbox) and the one it raises (in the peer's)
  const u64* wait_word = p.mbox + (sends ? mbox_credit(n, C, peer, w) : mbox_ready(C, peer, w));
  u64* raise_word = p.peer_mbox[peer] + (sends ? mbox_ready(C, r, w) : mbox_credit(n, C, r, w));
  const u64 slot = p.slot_bytes;
  for (int i = first; i < first + count; ++i) {
    const u64 bytes = a.bytes[i], nsl = p2p_nslices(bytes, slot);
    const int A = p2p_msg_pipes(bytes, slot, a.p2p_pipes);
    if (w >= A) continue;  // this message uses fewer pipelines: the pair's counters on w stay
    char* local = reinterpret_cast<char*>(a.ptr[i]);
    const bool vec = a.vec[i] != 0;
    for (u64 s = (u64)w; s < nsl; s += (u64)A) {
      const uint32_t len = (uint32_t)slice_len(bytes, slot, s);
      // sender: the slot is free once message seq - slots was consumed; receiver: the message landed
      const bool ok = sends ? (seq + 1 <= (u64)K || wave_wait_ge(wait_word, seq + 1 - K, ctl, lane))
                            : wave_wait_ge(wait_word, seq + 1, ctl, lane);
      if (!ok) {
        if (lane == 0) st_sys(p.peer_mbox[peer] + mbox_abort(n, C), abort_word(p));
        return;
      }
      char* at = local + s * slot;
      if (sends) {
        const rsrc_t out = make_rsrc(msg_slot(p, C, r, peer, w, seq), len);
        if (vec) move<P2pElem, kSum, true, kSend>(at, at, out, out, len, lane);
        else move<P2pElem, kSum, false, kSend>(at, at, out, out, len, lane);
        p2p_last_byte(true, at, out, len, lane);
      } else {
        acquire_sys(p.sys_fence);
        const rsrc_t in = make_rsrc(msg_slot(p, C, peer, r, w, seq), len);
        if (vec) move<P2pElem, kSum, true, kCopy>(at, at, in, in, len, lane);
        else move<P2pElem, kSum, false, kCopy>(at, at, in, in, len, lane);
        p2p_last_byte(false, at, in, len, lane);
      }
      drain_stores();  // every load of the slot has returned and every store has landed
      ++seq;
      if (lane == 0) {
        if (sends) publish(raise_word, seq, p.sys_fence);
        else st_sys(raise_word, seq);
      }
    }
  }
  if (lane == 0) *ctr = seq;
}

// ---------------------------------------------------------------- point to point on registered windows
// p2p_window_group: the launch of a group on a communicator with at least one registered window
// (Comm::p2p_group; with none, p2p_kernel above runs as it always did).  The mapping is p2p_kernel's:
// every directed pair on waves of its own, one per pipeline, a pair's operations in call order, the
// self pairs copied by their own waves.  What is new is one hand-off per message, from the device:
//
//  * Receiver, at the start of message m on pipeline w: lane 0 writes a DEST record into the SENDER's
//    mailbox (schedule.h mbox_dest_info / mbox_dest_tag, p2p.h P2pDest) -- three info words (st_sys),
//    drained, then the tag, the pair's message counter + 1 (publish).  The record says "direct:
//    window slot, byte offset, byte count" when the host found recvbuff inside a window with a table
//    slot, else "scratch: byte count".  The counters are monotone across calls, schedules and graph
//    replays, so a stale tag is always below the one a sender waits for.
//  * Sender: waits for the tag (wait_ge_spin: bounded, abort-aware), reads the record, and checks it
//    BEFORE it stores anything: the byte count equals its own (both paths), the slot is live in its
//    table, offset + bytes lies inside the window (p2p_dest_check).  A failure is the windows'
//    mismatch: kStatusMismatch claimed, the peer's ABORT raised with that cause, nothing written.
//  * Direct: pipeline w pushes slices w, w + A, ... of the message into dest + s * slot_bytes, all in
//    one push_pairs_vec run (the slices are its pairs: the next slice's loads leave before this one's
//    stores) -- 16-byte non-temporal loads of the own send, sc0 sc1 stores to the peer -- when source
//    and destination are both dword-aligned, which only the device knows: a wave-uniform branch;
//    else, and for each slice's last len % 16 bytes, 2-byte elements.  No CREDIT wait: no slot is
//    used.  The wave drains and raises READY ONCE, to seq + p2p_pipe_msgs: the sequence numbers the
//    scratch form of the same message would consume, so direct and scratch messages and collectives
//    follow each other on one pair in any order.  The receiver's wave waits for that READY and
//    returns CREDIT at the same value; it moves no data.  The pushed bytes are visible to the
//    receiver's stream work after its call as the read schedule's pushes are (file header).
//  * Scratch: p2p_kernel's per-slice protocol, unchanged.
__device__ __forceinline__ void p2p_give_up(const CollParams& p, const Ctl& c, int C, int peer, int lane, uint32_t seen) {
  if (lane != 0) return;
  if (seen && claim_first(c)) st_sys32(c.status, seen);
  st_sys(p.peer_mbox[peer] + mbox_abort(p.n, C), abort_word(p, seen));
}

// slices w, w + A, ... (`mine` of them) of a message of `bytes` from src into dst
__device__ __forceinline__ void p2p_push_direct(const char* src, char* dst, u64 bytes, u64 slot, int A, int w, int mine,
                                                int lane) {
  auto at = [&](int k) { return ((u64)w + (u64)k * (u64)A) * slot; };
  auto len_of = [&](int k) { return k < mine ? (uint32_t)slice_len(bytes, slot, (u64)w + (u64)k * (u64)A) : 0u; };
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | slot) & 3u) == 0;
  if (vec) {
    auto src_of = [&](int k) { return make_rsrc(src + (k < mine ? at(k) : 0), len_of(k) & ~15u); };
    auto dst_of = [&](int k) { return make_rsrc(dst + (k < mine ? at(k) : 0), len_of(k) & ~15u); };
    // (a full slice's vectors: a shorter last slice ends inside its resource, which drops the rest)
    const uint32_t nvec = (uint32_t)((bytes < slot ? bytes : slot) >> 4);
    if (nvec) push_pairs_vec<kDealV>(mine, src_of, dst_of, nvec, lane);
  }
  for (int k = 0; k < mine; ++k) {
    const uint32_t len = len_of(k), done = vec ? len & ~15u : 0u;
    if (done == len) continue;
    const rsrc_t s = make_rsrc(src + at(k), len), d = make_rsrc(dst + at(k), len);
    for (uint32_t i = done / 2 + (uint32_t)lane; i < len / 2; i += 64) Scal<2>::st(d, i * 2, Scal<2>::ld(s, i * 2));
    if ((len & 1u) && lane == 0) Scal<1>::st(d, len - 1, Scal<1>::ld(s, len - 1));  // (a one-byte datatype's odd count)
  }
}

__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) p2p_window_group(CollParams p, P2pWinArgs wa) {
  signal_start(p);
  const P2pArgs& a = wa.a;
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const int nwaves = a.npairs * a.pipes;
  if (b >= nwaves) {
    p2p_self_copies(a, b - nwaves, lane);
    return;
  }
  const int pair = b / a.pipes, w = b % a.pipes, C = p.pipes;
  const int n = p.n, r = p.rank, K = p.nslots;
  const int peer = a.pair_peer[pair], first = a.pair_first[pair], count = a.pair_count[pair];
  const bool sends = a.pair_send[pair] != 0;
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  u64* ctr = (sends ? p.tx_seq : p.rx_seq) + (u64)peer * C + w;
  u64 seq = uniform64(*ctr);
  const u64* wait_word = p.mbox + (sends ? mbox_credit(n, C, peer, w) : mbox_ready(C, peer, w));
  u64* raise_word = p.peer_mbox[peer] + (sends ? mbox_ready(C, r, w) : mbox_credit(n, C, r, w));
  // the DEST record of this (pair, pipeline): a receiver writes the sender's copy, a sender reads its own
  u64* dest_info = (sends ? p.mbox + mbox_dest_info(n, C, peer, w) : p.peer_mbox[peer] + mbox_dest_info(n, C, r, w));
  u64* dest_tag = dest_info + kFlagStride;
  const u64 slot = p.slot_bytes;
  u64 pushed = 0;  // messages this wave's pair pushed direct (counted on pipeline 0, which every message uses)
  for (int i = first; i < first + count; ++i) {
    const u64 bytes = a.bytes[i], nsl = p2p_nslices(bytes, slot);
    const int A = p2p_msg_pipes(bytes, slot, a.p2p_pipes);
    if (w >= A) continue;  // this message uses fewer pipelines: the pair's counters on w stay
    const u64 mine = p2p_pipe_msgs(bytes, slot, a.p2p_pipes, w);
    char* local = reinterpret_cast<char*>(a.ptr[i]);
    bool direct;
    char* dest = nullptr;
    if (!sends) {
      P2pDest d;
      d.tag = p2p_dest_tag(seq);
      d.direct = wa.wslot[i] != kP2pNoSlot ? 1u : 0u;
      d.slot = d.direct ? wa.wslot[i] : 0u;
      d.off = d.direct ? wa.woff[i] : 0;
      d.bytes = bytes;
      direct = d.direct != 0;
      if (lane == 0) {
        u64 info[kDestInfoWords];
        p2p_dest_encode(d, info);
#pragma unroll
        for (int k = 0; k < kDestInfoWords; ++k) st_sys(dest_info + k, info[k]);
        publish(dest_tag, d.tag, p.sys_fence);  // (drains the info words first)
      }
    } else {
      if (!wave_wait_ge(dest_tag, p2p_dest_tag(seq), ctl, lane)) {
        p2p_give_up(p, ctl, C, peer, lane, 0);
        return;
      }
      acquire_sys(p.sys_fence);  // (the record is read with system-scope loads of uncached memory)
      u64 info[kDestInfoWords];
#pragma unroll
      for (int k = 0; k < kDestInfoWords; ++k) info[k] = uniform64(ld_sys(dest_info + k));
      const P2pDest d = p2p_dest_decode(info, uniform64(ld_sys(dest_tag)));
      const bool slot_ok = d.direct && d.slot < (uint32_t)kP2pWinSlots;
      const u64 wbase = slot_ok ? uniform64(wa.table->base[d.slot][peer]) : 0;
      const u64 wbytes = slot_ok ? uniform64(wa.table->bytes[d.slot]) : 0;
      if (d.tag != p2p_dest_tag(seq) || p2p_dest_check(d, bytes, wbase, wbytes) != kDestOk) {
        p2p_give_up(p, ctl, C, peer, lane, kStatusMismatch);
        return;
      }
      direct = d.direct != 0;
      dest = reinterpret_cast<char*>(wbase + d.off);
    }
    if (direct) {
      if (sends) {
        p2p_push_direct(local, dest, bytes, slot, A, w, (int)mine, lane);
        drain_stores();
        seq += mine;
        if (lane == 0) publish(raise_word, seq, p.sys_fence);
        if (w == 0) ++pushed;
      } else {
        if (!wave_wait_ge(wait_word, seq + mine, ctl, lane)) {
          p2p_give_up(p, ctl, C, peer, lane, 0);
          return;
        }
        acquire_sys(p.sys_fence);
        seq += mine;
        if (lane == 0) st_sys(raise_word, seq);
      }
      continue;
    }
    const bool vec = a.vec[i] != 0;
    for (u64 s = (u64)w; s < nsl; s += (u64)A) {  // p2p_kernel's slice loop
      const uint32_t len = (uint32_t)slice_len(bytes, slot, s);
      const bool ok = sends ? (seq + 1 <= (u64)K || wave_wait_ge(wait_word, seq + 1 - K, ctl, lane))
                            : wave_wait_ge(wait_word, seq + 1, ctl, lane);
      if (!ok) {
        p2p_give_up(p, ctl, C, peer, lane, 0);
        return;
      }
      char* at = local + s * slot;
      if (sends) {
        const rsrc_t out = make_rsrc(msg_slot(p, C, r, peer, w, seq), len);
        if (vec) move<P2pElem, kSum, true, kSend>(at, at, out, out, len, lane);
        else move<P2pElem, kSum, false, kSend>(at, at, out, out, len, lane);
        p2p_last_byte(true, at, out, len, lane);
      } else {
        acquire_sys(p.sys_fence);
        const rsrc_t in = make_rsrc(msg_slot(p, C, peer, r, w, seq), len);
        if (vec) move<P2pElem, kSum, true, kCopy>(at, at, in, in, len, lane);
        else move<P2pElem, kSum, false, kCopy>(at, at, in, in, len, lane);
        p2p_last_byte(false, at, in, len, lane);
      }
      drain_stores();
      ++seq;
      if (lane == 0) {
        if (sends) publish(raise_word, seq, p.sys_fence);
        else st_sys(raise_word, seq);
      }
    }
  }
  if (lane == 0) {
    *ctr = seq;
    if (pushed) {  // this pair's only writer: the launches of one communicator run one after another
      const u64 total = wa.table->direct_sends[peer] + pushed;
      wa.table->direct_sends[peer] = total;
      st_sys(wa.host_sends + peer, total);
    }
  }
}

// ---------------------------------------------------------------- read schedule, grid form
// mncclAlgoReadGrid / MINI_NCCL_ALGO=read_grid, and auto's large read calls since 5.1
// (schedule.h read_grid_form): the push form of a large call (read_grid_fits) as three launches on
// the call's stream --
// read_start_kernel (one wave, pipeline 0: START to every peer, wait for theirs, then the device
// word `go` = this call), read_grid_kernel (the fold with no flag in sight: one one-wave
// workgroup per 1 KiB of my chunk, dispatched in address order, gone when done) and
// read_done_kernel (one wave: DONE to every peer, wait for theirs).  Why: the persistent kernel's
// long-lived waves move a 1:1 read:write stream at 72-80 % of HBM depending on where the buffers
// landed physically, while the dispatcher's one-batch workgroups held 77-81 % on every placement
// (tools/mix_probe.hip, profiles/r4_mix_probe_alloc.txt); on the one-GPU proxy, with the
// workgroup size following the rank count (read_grid_vectors), 1.16-1.21x the persistent form at
// 2 / 4 ranks and equal at 3 / 5 / 6 / 8 (profiles/r5_read_vs_grid_forms*.txt,
// r5_bench_n{2,4,8}_auto_grid.json); the node's bench measures both (schedules.read_grid).  The
// protocol is the push form's with one pipeline and one iteration
// (START, DONE: read_msgs_per_call(1) messages on pipeline 0's counters), which the simulator
// checks for a one-slice read call.  Stream order does the rest: the grid starts after START is
// through (its workgroups still check `go`: after a failed START they must not touch a peer's
// buffers), and every wave drains its stores before it ends, so when DONE is raised every load of
// a peer's send has returned and every push has been acknowledged by the peer's memory.
__global__ void __launch_bounds__(64) read_start_kernel(CollParams p) {
  signal_start(p);
  const int lane = threadIdx.x, n = p.n, r = p.rank, C = p.pipes;
  copy_tail(p, 0, lane);
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  const bool peer = lane < n && lane != r;
  const u64 tx = peer ? p.tx_seq[(u64)lane * C] : 0, rx = peer ? p.rx_seq[(u64)lane * C] : 0;
  send_start(p, C, lane, tx + 1, 0);
  uint32_t seen = 0;
  const bool ok = wave_wait_peers(p.mbox + mbox_ready(C, lane, 0), rx + 1, peer, ctl, lane, true) &&
                  starts_agree(p, ctl, C, lane, 0, &seen);
  // 0 after a failed START (a graph replay reuses call_seq: the word must not keep a stale "go")
  if (lane == 0) *p.go = ok ? p.call_seq : 0u;
  if (!ok && lane == 0)
    for (int k = 1; k < n; ++k) st_sys(p.peer_mbox[direct_peer(n, r, k)] + mbox_abort(n, C), abort_word(p, seen));
}

// one batch of V vectors per lane of my chunk: the peers' slices of it loaded together (G peer
// slots, as read_fold_all), folded in ring order, stored into my recv and pushed into every
// peer's recv (the push order rotated by workgroup so the workgroups' stores spread over the links)
template <typename T, int OPC, int G, int V>
__device__ __forceinline__ void grid_body(const CollParams& p) {
  if (*p.go != p.call_seq) return;  // START failed: the peers' buffers are not ours to touch
  constexpr uint32_t B = 64u * 16u * V;
  const uint32_t batch = blockIdx.x;
  const uint64_t off = (uint64_t)batch * B;
  if (off >= p.chunk_bytes) return;
  const int n = p.n, r = p.rank, lane = (int)threadIdx.x;
  const uint32_t len = (uint32_t)(p.chunk_bytes - off < B ? p.chunk_bytes - off : B);
  const uint64_t coff = (uint64_t)r * p.chunk_bytes + off;
  const rsrc_t loc = make_rsrc(p.send + coff, len), out = make_rsrc(p.recv + coff, len);
  v4u x[G][V], a[V];
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (g + 1 < n) {
      const rsrc_t in = make_rsrc(p.peer_send[direct_peer(n, r, 1 + g)] + coff, len);
#pragma unroll
      for (int u = 0; u < V; ++u) x[g][u] = ld_slot16(in, (uint32_t)(u * 64 + lane) * 16);
    }
#pragma unroll
  for (int u = 0; u < V; ++u) a[u] = ld_nt16(loc, (uint32_t)(u * 64 + lane) * 16);
#pragma unroll
  for (int u = 0; u < V; ++u) a[u] = prescale16<T, OPC>(a[u], p.scale);
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (g + 1 < n) {
#pragma unroll
      for (int u = 0; u < V; ++u) a[u] = reduce16<T, OPC>(prescale16<T, OPC>(x[g][u], p.scale), a[u]);
    }
#pragma unroll
  for (int u = 0; u < V; ++u) st_slot16(out, (uint32_t)(u * 64 + lane) * 16, a[u]);
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (g + 1 < n) {
      const int q = direct_peer(n, r, 1 + (int)((g + batch) % (unsigned)(n - 1)));
      const rsrc_t po = make_rsrc(p.peer_recv[q] + coff, len);
#pragma unroll
      for (int u = 0; u < V; ++u) st_slot16(po, (uint32_t)(u * 64 + lane) * 16, a[u]);
    }
  drain_stores();  // every push acknowledged by the peer's memory before this wave ends
}
template <typename T, int OPC, int G, int V>
__global__ void __launch_bounds__(64) read_grid_kernel(CollParams p) {
  grid_body<T, OPC, G, V>(p);
}
template <typename T, int OPC, int G, int V>
__global__ void __launch_bounds__(64) fp8_grid(CollParams p) {
  grid_body<T, OPC, G, V>(p);
}

__global__ void __launch_bounds__(64) read_done_kernel(CollParams p) {
  if (*p.go != p.call_seq) return;  // START failed and already raised the peers' ABORT words
  const int lane = threadIdx.x, n = p.n, r = p.rank, C = p.pipes;
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  const bool peer = lane < n && lane != r;
  const u64 mpc = read_msgs_per_call(1);
  const u64 tx = peer ? p.tx_seq[(u64)lane * C] : 0, rx = peer ? p.rx_seq[(u64)lane * C] : 0;
  if (p.sys_fence && lane == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (peer) {
    st_sys(p.peer_mbox[lane] + mbox_credit(n, C, r, 0), rx + mpc);
    st_sys(p.peer_mbox[lane] + mbox_ready(C, r, 0), tx + mpc);
  }
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, 0), rx + mpc, peer, ctl, lane, false)) {
    if (lane == 0)
      for (int k = 1; k < n; ++k) st_sys(p.peer_mbox[direct_peer(n, r, k)] + mbox_abort(n, C), abort_word(p));
    return;
  }
  if (peer) {
    p.tx_seq[(u64)lane * C] = tx + mpc;
    p.rx_seq[(u64)lane * C] = rx + mpc;
  }
}

// ---------------------------------------------------------------- one-shot kernel
// Small calls (schedule.h oneshot_fits): one hand-off instead of the ring's 2(n-1) dependent
// ones.  Pipeline w = s * n + c owns slice s of chunk c: it stores that piece of its send into
// every peer's scratch slot -- one message per (pair, pipeline) on the same FIFOs, READY words,
// credits and counters as the ring (calls of either schedule follow each other freely) -- and,
// once every peer's piece is in, folds the piece of the result itself in ring order: x_c, then
// acc = op(x_q, acc) for q = c+1, ..., c-1 (the read schedule's order, the reference ring's
// association), so every rank computes every element exactly as the ring does.  The n
// pipelines of a slice run side by side: a 4 KiB call at 8 ranks is 8 waves, each one piece
// out, one flag round, one fold.  Costs (n-1) x the call's bytes out per rank: small calls only.
template <typename T, int OPC, bool VEC>
__device__ __forceinline__ void oneshot_body(const CollParams& p) {
  signal_start(p);
  const WaveId id = wave_id();
  const int lane = id.lane, w = id.w, C = p.pipes, wv = id.wv;
  const int n = p.n, r = p.rank, K = p.nslots;
  copy_tail(p, w, lane);
  __shared__ u64 s_tx[kMaxWaves][kMaxRanks], s_rx[kMaxWaves][kMaxRanks];
  u64* tx = s_tx[wv];
  u64* rx = s_rx[wv];
  const Ctl ctl{p.status, p.host_abort, p.mbox + mbox_abort(n, C), p.timeout_ticks, p.mbox, p.claim};
  if (lane < n) {
    tx[lane] = p.tx_seq[(u64)lane * C + w];
    rx[lane] = p.rx_seq[(u64)lane * C + w];
  }
  __builtin_amdgcn_wave_barrier();
  const bool peer = lane < n && lane != r;  // lane q speaks for peer q
  const u64 mytx = tx[lane < n ? lane : 0], myrx = rx[lane < n ? lane : 0];
  const int c = w % n;
  const u64 s = (u64)(w / n);
  const uint32_t len = (uint32_t)slice_len(p.chunk_bytes, p.slice_bytes, s);
  const u64 coff = (u64)c * p.chunk_bytes + s * p.slice_bytes;
  const uint32_t nvec = VEC ? len >> 4 : 0;
  typedef typename Scal<sizeof(T)>::U U;
  const uint32_t ne = len / (uint32_t)sizeof(T), e0 = nvec * 16 / (uint32_t)sizeof(T);
  const rsrc_t mine = make_rsrc(p.send + coff, len);
  // my message's slot in every peer must be free (the peer consumed message tx - slots)
  if (!wave_wait_peers(p.mbox + mbox_credit(n, C, lane, w), mytx + 1 - (u64)K, peer && mytx + 1 > (u64)K, ctl, lane,
                       false))
    goto aborted;
  // my piece into every peer's slot
  for (uint32_t i = (uint32_t)lane; i < nvec; i += 64) {
    const v4u v = ld_slot16(mine, i * 16);
    for (int k = 1; k < n; ++k) {
      const int q = direct_peer(n, r, k);
      st_slot16(make_rsrc(msg_slot(p, C, r, q, w, tx[q]), len), i * 16, v);
    }
  }
  for (uint32_t e = e0 + (uint32_t)lane; e < ne; e += 64) {
    const U v = Scal<sizeof(T)>::ld(mine, e * (uint32_t)sizeof(T));
    for (int k = 1; k < n; ++k) {
      const int q = direct_peer(n, r, k);
      Scal<sizeof(T)>::st(make_rsrc(msg_slot(p, C, r, q, w, tx[q]), len), e * (uint32_t)sizeof(T), v);
    }
  }
  drain_stores();
  if (p.sys_fence && lane == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (peer) st_sys(p.peer_mbox[lane] + mbox_ready(C, r, w), mytx + 1);
  // every peer's piece, then the fold: in[k] = rank c + k's piece (my own send for me)
  if (!wave_wait_peers(p.mbox + mbox_ready(C, lane, w), myrx + 1, peer, ctl, lane, true)) goto aborted;
  acquire_sys(p.sys_fence);
  if (len) {
    rsrc_t in[kMaxRanks];
#pragma unroll
    for (int k = 0; k < kMaxRanks; ++k)
      if (k < n) {
        const int q = mod_n(c + k, n);
        in[k] = q == r ? mine : make_rsrc(msg_slot(p, C, q, r, w, rx[q]), len);
      }
    const rsrc_t out = make_rsrc(p.recv + coff, len);
    for (uint32_t i = (uint32_t)lane; i < nvec; i += 64) {
      v4u x[kMaxRanks];
#pragma unroll
      for (int k = 0; k < kMaxRanks; ++k)
        if (k < n) x[k] = ld_slot16(in[k], i * 16);
      v4u acc = x[0];
#pragma unroll
      for (int k = 1; k < kMaxRanks; ++k)
        if (k < n) acc = reduce16<T, OPC>(x[k], acc);
      st_nt16(out, i * 16, acc);
    }
    for (uint32_t e = e0 + (uint32_t)lane; e < ne; e += 64) {
      U x[kMaxRanks];
#pragma unroll
      for (int k = 0; k < kMaxRanks; ++k)
        if (k < n) x[k] = Scal<sizeof(T)>::ld(in[k], e * (uint32_t)sizeof(T));
      U acc = x[0];
#pragma unroll
      for (int k = 1; k < kMaxRanks; ++k)
        if (k < n) acc = __builtin_bit_cast(U, Op<T, OPC>::f(__builtin_bit_cast(T, x[k]), __builtin_bit_cast(T, acc)));
      Scal<sizeof(T)>::st(out, e * (uint32_t)sizeof(T), acc);
    }
  }
  drain_stores();  // every load of the peers' pieces has returned: their slots are free again
  if (peer) {
    st_sys(p.peer_mbox[lane] + mbox_credit(n, C, r, w), myrx + 1);
    p.tx_seq[(u64)lane * C + w] = mytx + 1;
    p.rx_seq[(u64)lane * C + w] = myrx + 1;
  }
  return;
aborted:
  if (lane == 0)
    for (int k = 1; k < n; ++k) st_sys(p.peer_mbox[direct_peer(n, r, k)] + mbox_abort(n, C), abort_word(p));
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) oneshot_kernel(CollParams p) {
  oneshot_body<T, OPC, VEC>(p);
}
template <typename T, int OPC, bool VEC>
__global__ void __launch_bounds__(kMaxThreads, kMinWavesPerSimd) fp8_oneshot(CollParams p) {
  oneshot_body<T, OPC, VEC>(p);
}

// ---------------------------------------------------------------- local reduce
// One 16-byte vector per lane, one wave per workgroup, one workgroup per 1 KiB of output,
// non-temporal loads and stores (the bytes are touched once).  Measured on MI355X for
// a <- a + b over 1 GiB fp32 (tools/lr_sweep.hip, interleaved rounds): 6.72 TB/s = 84 % of
// the 8 TB/s spec, vs 5.84 TB/s for a 4096-block grid-stride loop with 4 vectors per lane
// and 5.27 TB/s with plain (temporal) loads/stores.  Short-lived single-wave workgroups
// let the dispatcher keep every CU's memory pipeline full without a tail.
// The three kernels are stamped twice, under the names they always had for the five wider datatypes
// and under fp8_local_* for the fp8 types (instantiation sets are pinned by name; as whole kernels,
// not over a shared body function: inlined from one, the grid-stride forms read blockDim another way
// and the flagship kernel must compile to what it was).
//   VECK: one vector per lane; GSK: grid-stride form for buffers beyond 2^32 threads of the exact grid
//   (> 64 GiB); ELEMK: element by element (the last bytes % 16, and buffers that are not dword-aligned)
#define MNCCL_LOCAL_KERNELS(VECK, GSK, ELEMK)                                                                          \
  template <typename T, int OPC>                                                                                       \
  __global__ void __launch_bounds__(64) VECK(char* __restrict__ out, const char* __restrict__ a,                       \
                                             const char* __restrict__ b, u64 nvec) {                                   \
    const u64 i = (u64)blockIdx.x * 64 + threadIdx.x;                                                                  \
    if (i < nvec) {                                                                                                    \
      const v4u x = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(a) + i);                                   \
      const v4u y = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(b) + i);                                   \
      __builtin_nontemporal_store(reduce16<T, OPC>(x, y), reinterpret_cast<v4u*>(out) + i);                            \
    }                                                                                                                  \
  }                                                                                                                    \
  template <typename T, int OPC>                                                                                       \
  __global__ void __launch_bounds__(256) GSK(char* __restrict__ out, const char* __restrict__ a,                       \
                                             const char* __restrict__ b, u64 nvec) {                                   \
    const u64 stride = (u64)gridDim.x * blockDim.x;                                                                    \
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {                                  \
      const v4u x = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(a) + i);                                   \
      const v4u y = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(b) + i);                                   \
      __builtin_nontemporal_store(reduce16<T, OPC>(x, y), reinterpret_cast<v4u*>(out) + i);                            \
    }                                                                                                                  \
  }                                                                                                                    \
  template <typename T, int OPC>                                                                                       \
  __global__ void __launch_bounds__(256) ELEMK(T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,  \
                                               u64 n) {                                                                \
    const u64 stride = (u64)gridDim.x * blockDim.x;                                                                    \
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = Op<T, OPC>::f(a[i], b[i]);   \
  }
MNCCL_LOCAL_KERNELS(local_reduce_vec, local_reduce_vec_gs, local_reduce_scalar)
MNCCL_LOCAL_KERNELS(fp8_local_vec, fp8_local_gs, fp8_local_elem)
#undef MNCCL_LOCAL_KERNELS

// kPreMulSum on a communicator of one rank: the call is no copy but out[i] = round_T(s * in[i]), the
// same single rounding the folds apply (Scale).  out may be in (in place): an element is read and
// written by one thread.  (Stamped twice, as the local-reduce kernels are.)
#define MNCCL_SCALE_KERNEL(NAME)                                                                                  \
  template <typename T>                                                                                           \
  __global__ void __launch_bounds__(256) NAME(T* out, const T* in, u64 n, u64 s) {                                \
    const u64 stride = (u64)gridDim.x * blockDim.x;                                                               \
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = Scale<T>::f(s, in[i]);  \
  }
MNCCL_SCALE_KERNEL(scale_kernel)
MNCCL_SCALE_KERNEL(fp8_scale)
#undef MNCCL_SCALE_KERNEL

// ---------------------------------------------------------------- link probe
struct ProbeArgs {
  char* local;
  char* remote[kMaxRanks];
  int nremote;
  uint64_t bytes;
};

// cache-policy bits of the probe's remote accesses (kProbe* in kernels.h): the hot path's
// sc0 sc1, non-temporal, or the default policy
template <int FORM> struct ProbeAux;
template <> struct ProbeAux<kProbeSys> { static constexpr int v = kAuxSys; };
template <> struct ProbeAux<kProbeNt> { static constexpr int v = 2; };
template <> struct ProbeAux<kProbePlain> { static constexpr int v = 0; };

// blocks [d * per, (d+1) * per) move `bytes` between `local` and remote d; 8 x 16 B per lane in
// flight.  PULL = false: local -> remote (the schedules' pushes); true: remote -> local (loads
// over the link, for comparison).
template <int FORM, bool PULL>
__global__ void __launch_bounds__(256) link_probe_kernel(ProbeArgs a) {
  constexpr int AUX = ProbeAux<FORM>::v;
  const int per = gridDim.x / a.nremote;
  const int d = blockIdx.x / per, b = blockIdx.x % per;
  if (d >= a.nremote) return;
  const uint64_t nvec = a.bytes / 16;
  const rsrc_t rem = make_rsrc(a.remote[d], (uint32_t)a.bytes);
  const rsrc_t loc = make_rsrc(a.local, (uint32_t)a.bytes);
  for (uint64_t base = (uint64_t)b * 256 * 8 + threadIdx.x; base < nvec; base += (uint64_t)per * 256 * 8) {
    v4u v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint64_t i = base + (uint64_t)u * 256;
      if (i < nvec)
        v[u] = PULL ? __builtin_amdgcn_raw_buffer_load_b128(rem, (uint32_t)(i * 16), 0, AUX)
                    : __builtin_amdgcn_raw_buffer_load_b128(loc, (uint32_t)(i * 16), 0, 2);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint64_t i = base + (uint64_t)u * 256;
      if (i < nvec) {
        if (PULL) __builtin_amdgcn_raw_buffer_store_b128(v[u], loc, (uint32_t)(i * 16), 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b128(v[u], rem, (uint32_t)(i * 16), 0, AUX);
      }
    }
  }
}

hipError_t launch_link_probe(char* local, char* const* remote, int nremote, uint64_t bytes, int form, bool pull,
                             hipStream_t st) {
  if (nremote < 1 || nremote > kMaxRanks || bytes == 0 || bytes > 0xffffffffull) return hipErrorInvalidValue;
  ProbeArgs a;
  a.local = local;
  for (int i = 0; i < kMaxRanks; ++i) a.remote[i] = i < nremote ? remote[i] : nullptr;
  a.nremote = nremote;
  a.bytes = bytes;
  const int per = 256 / nremote > 0 ? 256 / nremote : 1;
  const dim3 g(per * nremote), blk(256);
#define PROBE_CASE(F)                                                        \
  case F:                                                                    \
    if (pull) hipLaunchKernelGGL((link_probe_kernel<F, true>), g, blk, 0, st, a); \
    else hipLaunchKernelGGL((link_probe_kernel<F, false>), g, blk, 0, st, a);     \
    break;
  switch (form) {
    PROBE_CASE(kProbeSys) PROBE_CASE(kProbeNt) PROBE_CASE(kProbePlain)
    default: return hipErrorInvalidValue;
  }
#undef PROBE_CASE
  return hipGetLastError();
}

// ---------------------------------------------------------------- dispatch
// A runtime dtype / op / vec / element size becomes a tag whose type carries the constant; the
// callee (a generic lambda) names the kernel template with it.  An unknown value is refused.
template <typename T> struct TypeTag { using type = T; };
template <int I> using IntTag = std::integral_constant<int, I>;

template <typename F>
static hipError_t for_dtype(int dtype, F&& f) {
  switch (dtype) {
    case kF32: return f(TypeTag<float>{});
    case kF64: return f(TypeTag<double>{});
    case kI32: return f(TypeTag<int32_t>{});
    case kF16: return f(TypeTag<_Float16>{});
    case kBF16: return f(TypeTag<bf16_t>{});
    default: return hipErrorInvalidValue;
  }
}

// the fp8 types: dispatched apart, to entry points of their own (the fp8_* / byte_* kernels), so
// that for_dtype and for_elem_size keep instantiating exactly the kernels they always did
static bool is_fp8(int dtype) { return dtype == kF8E4M3 || dtype == kF8E5M2; }

template <typename F>
static hipError_t for_fp8(int dtype, F&& f) {
  switch (dtype) {
    case kF8E4M3: return f(TypeTag<e4m3_t>{});
    case kF8E5M2: return f(TypeTag<e5m2_t>{});
    default: return hipErrorInvalidValue;
  }
}

template <typename F>
static hipError_t for_op(int op, F&& f) {
  switch (op) {
    case kSum: return f(IntTag<kSum>{});
    case kProd: return f(IntTag<kProd>{});
    case kMax: return f(IntTag<kMax>{});
    case kMin: return f(IntTag<kMin>{});
    default: return hipErrorInvalidValue;
  }
}

// the fp8 family's ops: the four built-ins and kPreMulSum (one template parameter, no second entry point)
template <typename F>
static hipError_t for_fp8_op(int op, F&& f) {
  return op == kPreMulSum ? f(IntTag<kPreMulSum>{}) : for_op(op, f);
}

// (element size 1 is not here: the callers send it to the byte_* kernels)
template <typename F>
static hipError_t for_elem_size(int dtype, F&& f) {
  switch (dtype_size(dtype)) {
    case 2: return f(IntTag<2>{});
    case 4: return f(IntTag<4>{});
    case 8: return f(IntTag<8>{});
    default: return hipErrorInvalidValue;
  }
}

template <typename F>
static hipError_t for_vec(bool vec, F&& f) {
  return vec ? f(std::true_type{}) : f(std::false_type{});
}

// the kernels that fold: f(type, op, vec)
template <typename F>
static hipError_t for_type_op_vec(int dtype, int op, bool vec, F&& f) {
  return for_dtype(dtype, [&](auto t) {
    return for_op(op, [&](auto o) { return for_vec(vec, [&](auto v) { return f(t, o, v); }); });
  });
}

// the kernels that only copy: f(element size, vec)
template <typename F>
static hipError_t for_size_vec(int dtype, bool vec, F&& f) {
  return for_elem_size(dtype, [&](auto e) { return for_vec(vec, [&](auto v) { return f(e, v); }); });
}

template <typename T, int OPC>
static hipError_t local_for(void* out, const void* a, const void* b, u64 count, hipStream_t st) {
  // 16-byte vectors over the body whenever the three buffers are dword-aligned (4-byte-aligned
  // dwordx4 accesses are valid on gfx950), then the last (bytes % 16) bytes element-wise
  const bool vec = ((uintptr_t)out | (uintptr_t)a | (uintptr_t)b) % 4 == 0;
  const u64 nvec = vec ? count * sizeof(T) / 16 : 0;
  const u64 done = nvec * 16 / sizeof(T);
  const u64 kMaxExactBlocks = (1ull << 31) / 64;  // keep the exact grid under 2^31 threads
  // (the fp8 types: the same three kernels under their fp8_local_* names)
  constexpr bool f8 = IsFp8<T>::value;
  const dim3 exact((unsigned)((nvec + 63) / 64)), rest((unsigned)std::min<u64>((count - done + 255) / 256, 16384));
  if (nvec && (nvec + 63) / 64 <= kMaxExactBlocks) {
    if constexpr (f8) hipLaunchKernelGGL((fp8_local_vec<T, OPC>), exact, dim3(64), 0, st, (char*)out, (const char*)a, (const char*)b, nvec);
    else hipLaunchKernelGGL((local_reduce_vec<T, OPC>), exact, dim3(64), 0, st, (char*)out, (const char*)a, (const char*)b, nvec);
  } else if (nvec) {
    if constexpr (f8) hipLaunchKernelGGL((fp8_local_gs<T, OPC>), dim3(16384), dim3(256), 0, st, (char*)out, (const char*)a, (const char*)b, nvec);
    else hipLaunchKernelGGL((local_reduce_vec_gs<T, OPC>), dim3(16384), dim3(256), 0, st, (char*)out, (const char*)a, (const char*)b, nvec);
  }
  if (count > done) {
    if constexpr (f8) hipLaunchKernelGGL((fp8_local_elem<T, OPC>), rest, dim3(256), 0, st, (T*)out + done, (const T*)a + done, (const T*)b + done, count - done);
    else hipLaunchKernelGGL((local_reduce_scalar<T, OPC>), rest, dim3(256), 0, st, (T*)out + done, (const T*)a + done, (const T*)b + done, count - done);
  }
  return hipGetLastError();
}

hipError_t preload_kernels() {
  // asking for any kernel's attributes makes the runtime load the whole code object for this device
  hipFuncAttributes attr;
  return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&read_start_kernel));
}

template <typename K>
static hipError_t launch_on(K kernel, int C, int nt, const CollParams& p, hipStream_t st) {
  hipLaunchKernelGGL(kernel, dim3(C), dim3(nt), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_persistent(int kernel, int dtype, int op, bool vec, int C, int nt, const CollParams& p,
                             hipStream_t st) {
  const bool root_ok = p.root >= 0 && p.root < p.n;
  // K: the kernel of the four built-in ops; S: its entry point for kPreMulSum (no op parameter);
  // F: the fp8 types' entry point (all five ops).  B: a copy kernel's entry point for element size 1
#define FP8_FOLDS(F)                                                                                          \
  for_fp8(dtype, [&](auto t) {                                                                                \
    return for_fp8_op(op, [&](auto o) {                                                                       \
      return for_vec(vec, [&](auto v) {                                                                       \
        return launch_on(F<typename decltype(t)::type, decltype(o)::value, decltype(v)::value>, C, nt, p, st); \
      });                                                                                                     \
    });                                                                                                       \
  })
#define FOLDS(K, S, F)                                                                                        \
  (is_fp8(dtype) ? FP8_FOLDS(F) : op == kPreMulSum ? for_dtype(dtype, [&](auto t) {                                                          \
    return for_vec(vec, [&](auto v) { return launch_on(S<typename decltype(t)::type, decltype(v)::value>, C, nt, p, st); }); \
  }) : for_type_op_vec(dtype, op, vec, [&](auto t, auto o, auto v) {                                          \
    return launch_on(K<typename decltype(t)::type, decltype(o)::value, decltype(v)::value>, C, nt, p, st);   \
  }))
#define COPIES(K, B)                                                                                     \
  (dtype_size(dtype) == 1 ? for_vec(vec, [&](auto v) { return launch_on(B<decltype(v)::value>, C, nt, p, st); }) \
                          : for_size_vec(dtype, vec, [&](auto e, auto v) {                                 \
                              return launch_on(K<decltype(e)::value, decltype(v)::value>, C, nt, p, st);   \
                            }))
  switch (kernel) {
    case kKernelRing: return FOLDS(ring_kernel, scaled_ring, fp8_ring);
    case kKernelRead: return FOLDS(read_kernel, scaled_read, fp8_read);
        // (no one-shot form of kPreMulSum: Comm::collective routes such a call to the read schedule or the ring)
    case kKernelOneshot:
      if (op == kPreMulSum) return hipErrorInvalidValue;
      if (is_fp8(dtype))
        return for_fp8(dtype, [&](auto t) {
          return for_op(op, [&](auto o) {
            return for_vec(vec, [&](auto v) {
              return launch_on(fp8_oneshot<typename decltype(t)::type, decltype(o)::value, decltype(v)::value>, C, nt, p, st);
            });
          });
        });
      return for_type_op_vec(dtype, op, vec, [&](auto t, auto o, auto v) {
        return launch_on(oneshot_kernel<typename decltype(t)::type, decltype(o)::value, decltype(v)::value>, C, nt, p, st);
      });
    case kKernelScatterFold: return p.coll == kCollReduceScatter ? FOLDS(scatter_fold, scaled_scatter, fp8_scatter) : hipErrorInvalidValue;
    case kKernelGatherPush: return p.coll == kCollAllGather ? COPIES(gather_push, byte_gather) : hipErrorInvalidValue;
    case kKernelRootFold: return p.coll == kCollReduce && root_ok ? FOLDS(root_fold, scaled_root, fp8_root) : hipErrorInvalidValue;
    case kKernelRootRelay: return p.coll == kCollBroadcast && root_ok ? COPIES(root_relay, byte_relay) : hipErrorInvalidValue;
    case kKernelExchangePush: return p.coll == kCollAllToAll && p.n >= 2 ? COPIES(exchange_push, byte_exchange) : hipErrorInvalidValue;
    case kKernelCollectPush: return p.coll == kCollGather && root_ok && p.n >= 2 ? COPIES(collect_push, byte_collect) : hipErrorInvalidValue;
    case kKernelDealPush: return p.coll == kCollScatter && root_ok && p.n >= 2 ? COPIES(deal_push, byte_deal) : hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
#undef COPIES
#undef FOLDS
#undef FP8_FOLDS
}

hipError_t launch_vhalf(int dtype, int op, bool vec, int C, int nt, const CollParams& p, const VHalfArgs& v,
                        hipStream_t st) {
  if (p.n < 2 || v.bytes > p.chunk_bytes) return hipErrorInvalidValue;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(C), dim3(nt), 0, st, p, v);
    return hipGetLastError();
  };
  if (p.coll == kCollAllGatherV) {
    if (dtype_size(dtype) == 1) return for_vec(vec, [&](auto e) { return go(vhalf_byte<decltype(e)::value>); });
    return for_size_vec(dtype, vec, [&](auto e, auto w) { return go(vhalf_push<decltype(e)::value, decltype(w)::value>); });
  }
  if (p.coll != kCollReduceScatterV) return hipErrorInvalidValue;
  if (is_fp8(dtype))
    return for_fp8(dtype, [&](auto t) {
      return for_fp8_op(op, [&](auto o) {
        return for_vec(vec, [&](auto w) {
          return go(vhalf_fp8<typename decltype(t)::type, decltype(o)::value, decltype(w)::value>);
        });
      });
    });
  if (op == kPreMulSum)
    return for_dtype(dtype, [&](auto t) {
      return for_vec(vec, [&](auto w) { return go(scaled_vhalf<typename decltype(t)::type, decltype(w)::value>); });
    });
  return for_type_op_vec(dtype, op, vec, [&](auto t, auto o, auto w) {
    return go(vhalf_fold<typename decltype(t)::type, decltype(o)::value, decltype(w)::value>);
  });
}

hipError_t launch_varblock(int dtype, int C, int nt, const CollParams& p, const VarBlockArgs& v, hipStream_t st) {
  if (p.coll != kCollAllToAllV || p.n < 2) return hipErrorInvalidValue;
  if (dtype_size(dtype) == 1) {
    hipLaunchKernelGGL(byte_varblock, dim3(C), dim3(nt), 0, st, p, v);
    return hipGetLastError();
  }
  return for_elem_size(dtype, [&](auto e) {
    hipLaunchKernelGGL(varblock_push<decltype(e)::value>, dim3(C), dim3(nt), 0, st, p, v);
    return hipGetLastError();
  });
}

// the shapes both point-to-point kernels assume, checked before anything is launched: every index
// they form from the argument stays inside the argument's arrays and the communicator's layout
static bool p2p_shapes_ok(const CollParams& p, const P2pArgs& a) {
  const int waves = p2p_launch_waves(a);
  if (waves < 1 || a.npairs < 0 || a.npairs > kP2pMaxPairs || a.nself < 0 || a.self_waves < 0 ||
      a.self_waves > kP2pMaxSelfWaves || (a.nself == 0) != (a.self_waves == 0) || a.self_first < 0 ||
      a.self_first + 2 * a.nself > kMaxGroupOps)
    return false;
  if (a.npairs > 0) {
    if (p.n < 2 || p.n > kMaxRanks || p.nslots < 1 || !p.mbox || !p.tx_seq || !p.rx_seq || a.pipes < 1 ||
        a.pipes > a.p2p_pipes || a.p2p_pipes > p.pipes || p.slot_bytes == 0 || p.slot_bytes > kMaxSlice)
      return false;
    for (int i = 0; i < a.npairs; ++i)
      if (a.pair_peer[i] >= p.n || a.pair_peer[i] == p.rank || a.pair_count[i] < 1 ||
          a.pair_first[i] + a.pair_count[i] > a.self_first || !p.peer_mbox[a.pair_peer[i]] ||
          !p.peer_scratch[a.pair_peer[i]])
        return false;
  }
  return true;
}

hipError_t launch_p2p(const CollParams& p, const P2pArgs& a, hipStream_t st) {
  if (!p2p_shapes_ok(p, a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(p2p_kernel, dim3((unsigned)p2p_launch_waves(a)), dim3(64), 0, st, p, a);
  return hipGetLastError();
}

hipError_t launch_p2p_window(const CollParams& p, const P2pWinArgs& wa, hipStream_t st) {
  if (!p2p_shapes_ok(p, wa.a) || !wa.table || !wa.host_sends) return hipErrorInvalidValue;
  // a direct recv names a slot of the table (the sender checks the rest of the record on the device)
  for (int i = 0; i < wa.a.self_first; ++i)
    if (wa.wslot[i] != kP2pNoSlot && wa.wslot[i] >= kP2pWinSlots) return hipErrorInvalidValue;
  hipLaunchKernelGGL(p2p_window_group, dim3((unsigned)p2p_launch_waves(wa.a)), dim3(64), 0, st, p, wa);
  return hipGetLastError();
}

// One grid launch; which (G, V) exist: the rule's pairs (schedule.h read_grid_vectors: V = 1 up to
// 4 ranks, 2 past them) for every type and op, every pair for fp32 Sum (MINI_NCCL_GRID_VECTORS)
template <typename T, int OPC, int G, int V>
static hipError_t read_grid_launch(const CollParams& p, hipStream_t st) {
  constexpr bool tuned = std::is_same<T, float>::value && OPC == kSum;
  if constexpr (tuned || (V == 1 && G <= 4) || (V == 2 && G >= 4)) {
    // V 16-byte vectors per lane per workgroup: V KiB of the chunk each
    const uint64_t per_block = 1024ull * (uint64_t)V;
    const unsigned blocks = (unsigned)((p.chunk_bytes + per_block - 1) / per_block);
    if constexpr (IsFp8<T>::value) hipLaunchKernelGGL((fp8_grid<T, OPC, G, V>), dim3(blocks), dim3(64), 0, st, p);
    else hipLaunchKernelGGL((read_grid_kernel<T, OPC, G, V>), dim3(blocks), dim3(64), 0, st, p);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

template <typename T, int OPC>
static hipError_t read_grid_for(const CollParams& p, hipStream_t st, int vectors) {
  const int n = p.n;
  // MINI_NCCL_GRID_VECTORS: 1 / 2 / 4 vectors per lane for fp32 Sum (the bench's workload: the
  // node's sweep weighs them over xGMI); every other call follows the rule
  const bool tuned = vectors != 0 && std::is_same<T, float>::value && OPC == kSum;
  const int V = tuned ? vectors : read_grid_vectors(n);
  // the rule's instantiations hard-code V per rank count; a rule they do not match is
  // refused rather than launched with a grid sized for another V
  if (!tuned && V != (n <= 4 ? 1 : 2)) return hipErrorInvalidValue;
  // G peer slots by rank count, as read_fold_all's
  auto with_v = [&](auto v) {
    constexpr int VV = decltype(v)::value;
    return n == 2   ? read_grid_launch<T, OPC, 1, VV>(p, st)
           : n == 3 ? read_grid_launch<T, OPC, 2, VV>(p, st)
           : n <= 5 ? read_grid_launch<T, OPC, 4, VV>(p, st)
                    : read_grid_launch<T, OPC, 7, VV>(p, st);
  };
  return V == 1 ? with_v(IntTag<1>{}) : V == 2 ? with_v(IntTag<2>{}) : with_v(IntTag<4>{});
}

hipError_t launch_read_grid(int dtype, int op, const CollParams& p, hipStream_t st, int vectors) {
  // the shapes the grid kernel assumes, checked before anything is launched
  if (p.n < 2 || p.n > 8 || p.chunk_bytes % 16 || !p.go || !read_grid_fits(p.chunk_bytes, p.n, kReadGridFloor) ||
      (p.chunk_bytes + 1023) / 1024 > 0x7fffffffull || (read_grid_vectors(p.n) != 1 && read_grid_vectors(p.n) != 2) ||
      (vectors != 0 && vectors != 1 && vectors != 2 && vectors != 4))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(read_start_kernel, dim3(1), dim3(64), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  auto grid = [&](auto t) {
    using T = typename decltype(t)::type;
    if (op == kPreMulSum) return read_grid_for<T, kPreMulSum>(p, st, vectors);
    return for_op(op, [&](auto o) { return read_grid_for<T, decltype(o)::value>(p, st, vectors); });
  };
  e = is_fp8(dtype) ? for_fp8(dtype, grid) : for_dtype(dtype, grid);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(read_done_kernel, dim3(1), dim3(64), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_local_reduce(int dtype, int op, void* out, const void* local, const void* incoming, uint64_t count,
                               hipStream_t st) {
  if (count == 0) return hipSuccess;
  auto run = [&](auto t) {
    return for_op(op, [&](auto o) {
      return local_for<typename decltype(t)::type, decltype(o)::value>(out, local, incoming, count, st);
    });
  };
  return is_fp8(dtype) ? for_fp8(dtype, run) : for_dtype(dtype, run);
}

hipError_t launch_scale(int dtype, void* out, const void* in, uint64_t count, uint64_t scale, hipStream_t st) {
  if (count == 0) return hipSuccess;
  auto run = [&](auto t) {
    using T = typename decltype(t)::type;
    const dim3 grid((unsigned)std::min<u64>((count + 255) / 256, 16384));
    if constexpr (IsFp8<T>::value) hipLaunchKernelGGL(fp8_scale<T>, grid, dim3(256), 0, st, (T*)out, (const T*)in, (u64)count, (u64)scale);
    else hipLaunchKernelGGL(scale_kernel<T>, grid, dim3(256), 0, st, (T*)out, (const T*)in, (u64)count, (u64)scale);
    return hipGetLastError();
  };
  return is_fp8(dtype) ? for_fp8(dtype, run) : for_dtype(dtype, run);
}

bool dtype_supported(int dtype) { return dtype_size(dtype) != 0; }

int dtype_size(int dtype) {
  switch (dtype) {
    case kF32: case kI32: return 4;
    case kF64: return 8;
    case kF16: case kBF16: return 2;
    case kF8E4M3: case kF8E5M2: return 1;
    default: return 0;
  }
}

}  // namespace mnccl
