// api.cpp -- the C ABI (include/mini_nccl_api.h, include/mini_nccl_ext.h).
//
// Thin bridge, as the reference's src/api.cpp: argument checks in the reference's order
// and with its error codes, an exception firewall (no C++ exception crosses the ABI),
// dtype/op validation, one roctx range per all-reduce (the reference's NVTX range,
// api.cpp:142-151), then the communicator's hot path.
#include <hip/hip_runtime_api.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstddef>
#include <cstdio>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>

#include <cstring>

#include "comm.h"
#include "ipcreg.h"
#include "kernels.h"
#include "mini_nccl_api.h"
#include "mini_nccl_ext.h"
#include "p2p.h"

using mnccl::Comm;

namespace {

// reference api.cpp:101-128: Float/Int32/Double x Sum/Prod/Max/Min; this build adds
// Float16/Bfloat16 (build-defined parity).  Anything else -> error.
// ncclFloat8e4m3 / ncclFloat8e5m2 (mini_nccl_ext.h): the OCP fp8 types, wherever ncclBfloat16 is accepted.
bool dtype_ok(ncclDataType_t t) {
  return t == ncclFloat || t == ncclDouble || t == ncclInt32 || t == ncclFloat16 || t == ncclBfloat16 ||
         t == ncclFloat8e4m3 || t == ncclFloat8e5m2;
}
bool op_ok(ncclRedOp_t op) { return op == ncclSum || op == ncclProd || op == ncclMax || op == ncclMin; }

// The op of a collective that folds, after its datatype was found supported.  The four built-ins as
// they are and ncclAvg refused, both before the communicator is read; a value from
// MNCCL_FIRST_USER_OP up is looked up in the communicator: a handle of ncclRedOpCreatePreMulSum
// becomes kPreMulSum with its scalar's bits, an unknown one is ncclInternalError like any unsupported
// op, one created for another datatype ncclInvalidArgument.
ncclResult_t resolve_op(const char* what, const Comm* c, ncclDataType_t datatype, ncclRedOp_t op, int* kop,
                        uint64_t* scalar) {
  *scalar = 0;
  *kop = (int)op;
  if (op_ok(op)) return ncclSuccess;
  int made_for = 0;
  if ((int)op < MNCCL_FIRST_USER_OP || !c->redop_find((int)op, &made_for, scalar)) {
    fprintf(stderr, "[Mini-NCCL] %s Internal Error: unsupported RedOp\n", what);
    return ncclInternalError;
  }
  if (made_for != (int)datatype) {
    fprintf(stderr, "[Mini-NCCL] %s: the op was created for another datatype\n", what);
    return ncclInvalidArgument;
  }
  *kop = mnccl::kPreMulSum;
  return ncclSuccess;
}

// ncclGroupStart / ncclGroupEnd: the group being recorded, one per thread (ranks may run as threads
// of one process).  Groups nest by a depth counter; the outermost ncclGroupEnd launches.  The first
// error of an operation poisons the group: ncclGroupEnd returns it and launches nothing.
struct GroupState {
  int depth = 0;
  ncclResult_t err = ncclSuccess;
  Comm* comm = nullptr;  // the communicator and stream every operation of the group must name
  hipStream_t stream = nullptr;
  mnccl::P2pGroup ops;
};
thread_local GroupState g_group;

// a collective called while a group is open: deferred collectives are out of scope
bool group_open() { return g_group.depth > 0; }

struct RoctxRange {
  explicit RoctxRange(const char* m) { roctxRangePushA(m); }
  ~RoctxRange() { roctxRangePop(); }
};

}  // namespace

extern "C" {

const char* ncclGetErrorString(ncclResult_t result) {
  switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "unhandled hip error";
    case ncclSystemError: return "system error";
    case ncclInternalError: return "internal error";
    case ncclInvalidArgument: return "invalid argument";
    case ncclInvalidUsage: return "invalid usage";
    case ncclRemoteError: return "remote error";
    case ncclInProgress: return "in progress";
    default: return "unknown error";
  }
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nRanks, int rank, const char* ip) {
  if (!comm) return ncclInvalidArgument;
  if (rank == -1) {
    fprintf(stderr, "[Mini-NCCL] Hera auto-rank mode (rank == -1) is not supported by this build\n");
    return ncclInvalidUsage;
  }
  if (nRanks < 1 || rank < 0 || rank >= nRanks) return ncclInvalidArgument;
  try {
    Comm* c = new Comm(nRanks, rank, ip ? std::string(ip) : std::string("127.0.0.1"));
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
  } catch (const std::exception& e) {
    // every init failure is ncclSystemError, as in the reference (api.cpp:62-65): also a
    // configuration that differs between ranks, an unparsable MINI_NCCL_* value, nRanks > 16
    fprintf(stderr, "[Mini-NCCL] Init Failed: %s\n", e.what());
    return ncclSystemError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (!comm) return ncclInvalidArgument;
  try {
    delete reinterpret_cast<Comm*>(comm);
    return ncclSuccess;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t ncclCommUserRank(const ncclComm_t comm, int* rank) {
  if (!comm || !rank) return ncclInvalidArgument;
  *rank = reinterpret_cast<const Comm*>(comm)->rank();
  return ncclSuccess;
}

ncclResult_t ncclCommCount(const ncclComm_t comm, int* count) {
  if (!comm || !count) return ncclInvalidArgument;
  *count = reinterpret_cast<const Comm*>(comm)->nranks();
  return ncclSuccess;
}

ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                           ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  if (!comm || !sendbuff || !recvbuff) return ncclInvalidArgument;  // api.cpp:139
  if (count == 0) return ncclSuccess;                               // api.cpp:140
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclAllReduce");
  if (!dtype_ok(datatype)) {
    // the reference throws inside get_type_size / to_internal_op -> ncclInternalError (:182-185)
    fprintf(stderr, "[Mini-NCCL] AllReduce Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  int kop = 0;
  uint64_t scalar = 0;
  const ncclResult_t orc = resolve_op("AllReduce", reinterpret_cast<const Comm*>(comm), datatype, op, &kop, &scalar);
  if (orc != ncclSuccess) return orc;
  try {
    return reinterpret_cast<Comm*>(comm)->allreduce(sendbuff, recvbuff, count, (int)datatype, kop, stream, scalar);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] AllReduce Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// ------------------------------------------------------------------ extensions
// The all-reduce's two halves under NCCL's names and argument order (mini_nccl_ext.h): the same
// checks in the same order as ncclAllReduce above.
ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype,
                               ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  if (!comm || !sendbuff || !recvbuff) return ncclInvalidArgument;
  if (recvcount == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclReduceScatter");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] ReduceScatter Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  int kop = 0;
  uint64_t scalar = 0;
  const ncclResult_t orc = resolve_op("ReduceScatter", reinterpret_cast<const Comm*>(comm), datatype, op, &kop, &scalar);
  if (orc != ncclSuccess) return orc;
  try {
    return reinterpret_cast<Comm*>(comm)->reduce_scatter(sendbuff, recvbuff, recvcount, (int)datatype, kop, stream, scalar);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] ReduceScatter Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                           ncclComm_t comm, hipStream_t stream) {
  if (!comm || !sendbuff || !recvbuff) return ncclInvalidArgument;
  if (sendcount == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclAllGather");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] AllGather Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->all_gather(sendbuff, recvbuff, sendcount, (int)datatype, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] AllGather Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// The two rooted collectives (mini_nccl_ext.h).  The buffer a rank's role does not use may be NULL,
// so the buffers are checked where the communicator's rank and size are known (Comm::collective),
// with the root: after count == 0 and the datatype, as the header states.
ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, hipStream_t stream) {
  if (!comm) return ncclInvalidArgument;
  if (count == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclBroadcast");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] Broadcast Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->broadcast(sendbuff, recvbuff, count, (int)datatype, root, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] Broadcast Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op,
                        int root, ncclComm_t comm, hipStream_t stream) {
  if (!comm) return ncclInvalidArgument;
  if (count == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclReduce");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] Reduce Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  int kop = 0;
  uint64_t scalar = 0;
  const ncclResult_t orc = resolve_op("Reduce", reinterpret_cast<const Comm*>(comm), datatype, op, &kop, &scalar);
  if (orc != ncclSuccess) return orc;
  try {
    return reinterpret_cast<Comm*>(comm)->reduce(sendbuff, recvbuff, count, (int)datatype, kop, root, stream, scalar);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] Reduce Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// The all-to-all (mini_nccl_ext.h): the halves' checks in their order; the overlap of the two
// buffers is checked where the communicator's size is known (Comm::collective), after the datatype.
ncclResult_t ncclAllToAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclComm_t comm,
                          hipStream_t stream) {
  if (!comm || !sendbuff || !recvbuff) return ncclInvalidArgument;
  if (count == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclAllToAll");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] AllToAll Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->all_to_all(sendbuff, recvbuff, count, (int)datatype, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] AllToAll Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// Gather and scatter (mini_nccl_ext.h): the rooted collectives' checks in their order -- the large
// buffer may be NULL off the root, so the buffers are checked with the root where the
// communicator's rank and size are known (Comm::collective).
ncclResult_t ncclGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, int root,
                        ncclComm_t comm, hipStream_t stream) {
  if (!comm) return ncclInvalidArgument;
  if (sendcount == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclGather");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] Gather Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->gather(sendbuff, recvbuff, sendcount, (int)datatype, root, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] Gather Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t ncclScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype, int root,
                         ncclComm_t comm, hipStream_t stream) {
  if (!comm) return ncclInvalidArgument;
  if (recvcount == 0) return ncclSuccess;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclScatter");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] Scatter Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->scatter(sendbuff, recvbuff, recvcount, (int)datatype, root, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] Scatter Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// The variable all-to-all (mini_nccl_ext.h): the communicator and the four arrays, then the
// datatype; the buffers may be NULL on a rank whose counts are all zero, so they are checked with
// the counts where the communicator's size is known (Comm::all_to_all_v, varblock.h).
ncclResult_t ncclAllToAllv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[], void* recvbuff,
                           const size_t recvcounts[], const size_t rdispls[], ncclDataType_t datatype, ncclComm_t comm,
                           hipStream_t stream) {
  if (!comm || !sendcounts || !sdispls || !recvcounts || !rdispls) return ncclInvalidArgument;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclAllToAllv");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] AllToAllv Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->all_to_all_v(sendbuff, sendcounts, sdispls, recvbuff, recvcounts, rdispls,
                                                       (int)datatype, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] AllToAllv Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// The halves with per-rank counts (mini_nccl_ext.h): the communicator and the two arrays, the open
// group, then the datatype and the op; the data buffers may be NULL where the counts are zero, so
// they are checked with the counts where the communicator's rank and size are known (Comm::vhalf,
// vhalves.h).
ncclResult_t mncclAllGatherv(const void* sendbuff, size_t sendcount, void* recvbuff, const size_t recvcounts[],
                             const size_t rdispls[], ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  if (!comm || !recvcounts || !rdispls) return ncclInvalidArgument;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclAllGatherv");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] AllGatherv Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  try {
    return reinterpret_cast<Comm*>(comm)->all_gather_v(sendbuff, sendcount, recvbuff, recvcounts, rdispls, (int)datatype,
                                                       stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] AllGatherv Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t mncclReduceScatterv(const void* sendbuff, const size_t sendcounts[], const size_t sdispls[], void* recvbuff,
                                 size_t recvcount, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                                 hipStream_t stream) {
  if (!comm || !sendcounts || !sdispls) return ncclInvalidArgument;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  RoctxRange range("mini_ncclReduceScatterv");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] ReduceScatterv Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  int kop = 0;
  uint64_t scalar = 0;
  const ncclResult_t orc = resolve_op("ReduceScatterv", reinterpret_cast<const Comm*>(comm), datatype, op, &kop, &scalar);
  if (orc != ncclSuccess) return orc;
  try {
    return reinterpret_cast<Comm*>(comm)->reduce_scatter_v(sendbuff, sendcounts, sdispls, recvbuff, recvcount,
                                                           (int)datatype, kop, stream, scalar);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] ReduceScatterv Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// Point to point (mini_nccl_ext.h): the checks in the header's order.  Inside a group a call only
// records its operation; outside, it is a group of one and launches at once.
static ncclResult_t p2p_call(bool send, const void* buff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                             hipStream_t stream) {
  GroupState& gs = g_group;
  const bool grouped = gs.depth > 0;
  auto fail = [&](ncclResult_t rc) {
    if (grouped && gs.err == ncclSuccess) gs.err = rc;
    return rc;
  };
  if (!comm || (!buff && count != 0)) return fail(ncclInvalidArgument);
  if (count == 0) return ncclSuccess;  // both ends skip it: nothing recorded, matching stays consistent
  RoctxRange range(send ? "mini_ncclSend" : "mini_ncclRecv");
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] %s Internal Error: unsupported DataType\n", send ? "Send" : "Recv");
    return fail(ncclInternalError);
  }
  Comm* c = reinterpret_cast<Comm*>(comm);
  try {
    if (!grouped) {
      mnccl::P2pGroup one;
      const ncclResult_t rc = c->p2p_validate(one, false, send, peer, buff, count, (int)datatype);
      return rc != ncclSuccess ? rc : c->p2p_group(one, stream);
    }
    if (gs.comm && (gs.comm != c || gs.stream != stream)) {
      fprintf(stderr, "[Mini-NCCL] %s: every operation of a group must name the same communicator and stream\n",
              send ? "ncclSend" : "ncclRecv");
      return fail(ncclInvalidUsage);
    }
    const ncclResult_t rc = c->p2p_validate(gs.ops, true, send, peer, buff, count, (int)datatype);
    if (rc != ncclSuccess) return fail(rc);
    gs.comm = c;
    gs.stream = stream;
    return ncclSuccess;
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] %s Internal Error: %s\n", send ? "Send" : "Recv", e.what());
    return fail(ncclInternalError);
  } catch (...) {
    return fail(ncclSystemError);
  }
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
  return p2p_call(true, sendbuff, count, datatype, peer, comm, stream);
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
  return p2p_call(false, recvbuff, count, datatype, peer, comm, stream);
}

ncclResult_t ncclGroupStart(void) {
  ++g_group.depth;
  return ncclSuccess;
}

ncclResult_t ncclGroupEnd(void) {
  GroupState& gs = g_group;
  if (gs.depth == 0) return ncclInvalidUsage;
  if (--gs.depth > 0) return ncclSuccess;
  // the outermost end: take the group and leave the thread's state clean whatever happens below
  const GroupState done = gs;
  gs = GroupState();
  if (done.err != ncclSuccess) return done.err;  // poisoned: nothing is launched
  if (done.ops.nops == 0 || !done.comm) return ncclSuccess;
  RoctxRange range("mini_ncclGroupEnd");
  try {
    return done.comm->p2p_group(done.ops, done.stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] GroupEnd Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

// User-created reduction ops (mini_nccl_ext.h): the checks in the header's order.  The scalar is read
// here, on the host, before the call returns.
ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                      ncclScalarResidence_t residence, ncclComm_t comm) {
  if (!comm || !op || !scalar) return ncclInvalidArgument;
  if (!dtype_ok(datatype)) {
    fprintf(stderr, "[Mini-NCCL] RedOpCreatePreMulSum Internal Error: unsupported DataType\n");
    return ncclInternalError;
  }
  Comm* c = reinterpret_cast<Comm*>(comm);
  if (c->sticky_error() != ncclSuccess) return c->sticky_error();
  if (residence != ncclScalarHostImmediate) {
    fprintf(stderr, "[Mini-NCCL] ncclRedOpCreatePreMulSum: only ncclScalarHostImmediate is supported (the scalar travels "
            "to the kernels by value)\n");
    return ncclInvalidUsage;
  }
  uint64_t bits = 0;
  memcpy(&bits, scalar, (size_t)mnccl::dtype_size((int)datatype));  // (little-endian: the low bytes)
  int h = 0;
  const ncclResult_t rc = c->redop_create(&h, (int)datatype, bits);
  if (rc == ncclSuccess) *op = (ncclRedOp_t)h;
  return rc;
}

ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm) {
  if (!comm) return ncclInvalidArgument;
  return reinterpret_cast<Comm*>(comm)->redop_destroy((int)op);
}

// Sub-communicators (mini_nccl_ext.h): the checks in the header's order.  The first four read neither
// the communicator nor the network and leave *newcomm as it was; a refusal inside an open group does
// not poison the group.
ncclResult_t ncclCommSplit(ncclComm_t comm, int color, int key, ncclComm_t* newcomm, ncclConfig_t* config) {
  if (!comm || !newcomm) return ncclInvalidArgument;
  if (group_open()) return ncclInvalidUsage;  // no deferred collectives (mini_nccl_ext.h)
  if (config) {
    fprintf(stderr, "[Mini-NCCL] ncclCommSplit: only a NULL config is supported (the child takes its parent's)\n");
    return ncclInvalidUsage;
  }
  if (color < 0 && color != NCCL_SPLIT_NOCOLOR) return ncclInvalidArgument;
  RoctxRange range("mini_ncclCommSplit");
  Comm* child = nullptr;
  const ncclResult_t rc = reinterpret_cast<Comm*>(comm)->split(color, key, &child);  // never throws
  *newcomm = reinterpret_cast<ncclComm_t>(child);
  return rc;
}

ncclResult_t mncclLocalReduce(void* out, const void* local, const void* incoming, size_t count,
                              ncclDataType_t datatype, ncclRedOp_t op, hipStream_t stream) {
  if (!out || !local || !incoming) return ncclInvalidArgument;
  if (count == 0) return ncclSuccess;
  if (!dtype_ok(datatype) || !op_ok(op)) return ncclInternalError;
  try {
    return mnccl::local_reduce(out, local, incoming, count, (int)datatype, (int)op, stream);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] LocalReduce Internal Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t mncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError) {
  if (!comm || !asyncError) return ncclInvalidArgument;
  *asyncError = reinterpret_cast<Comm*>(comm)->async_error();
  return ncclSuccess;
}

// The legacy entry point writes the layout it was published with (before 300): a caller built
// against an older header is never written past the end of its struct; mncclCommGetInfoV gives
// the rest.
ncclResult_t mncclCommGetInfo(ncclComm_t comm, mncclCommInfo_t* info) {
  return mncclCommGetInfoV(comm, info, offsetof(mncclCommInfo_t, ipc_open_failures));
}

ncclResult_t mncclCommGetInfoV(ncclComm_t comm, void* out, size_t size) {
  if (!comm || !out) return ncclInvalidArgument;
  const Comm* c = reinterpret_cast<const Comm*>(comm);
  const mnccl::Config& k = c->config();
  mncclCommInfo_t full;
  memset(&full, 0, sizeof full);
  mncclCommInfo_t* info = &full;
  info->rank = c->rank();
  info->nranks = c->nranks();
  info->device = c->device();
  info->slice_bytes = k.slice_size;
  info->window = k.window_size;
  info->signal_batch = k.signal_batch;
  info->slots = k.slots;
  info->threads = k.threads;
  info->algo = c->algo();
  info->blocking = k.blocking;
  info->sys_fence = k.sys_fence;
  info->timeout_s = k.timeout_ms / 1000.0;
  info->scratch_bytes = c->scratch_bytes();
  info->tune_ms[0] = info->tune_ms[1] = 0.0;  // round 1's init-time calibration, removed in 0.3.1
  info->channels = c->workgroups();
  info->pipelines = c->wave_channels();
  info->ranks_on_device = c->ranks_on_device();
  info->slot_bytes = c->wave_slice();
  info->last_algo = c->last_algo();
  info->peer_mappings = c->peer_mappings();
  info->scratch_algo = mncclAlgoRing;  // the read schedule's fallback
  info->calib_choice = -1;              // MINI_NCCL_CALIBRATE was removed in 400
  info->calib_ms[0] = info->calib_ms[1] = 0.0;
  info->ipc_open_failures = mnccl::ipc::open_failures();
  info->read_map_failures = c->peer_buffers().map_failures();
  info->read_rounds = c->peer_buffers().agreements();
  info->closed_freed = c->peer_buffers().closed_freed();
  info->live_exports = mnccl::ipc::live_exports();
  info->cap_refusals = mnccl::ipc::cap_refusals();
  info->liveness_queries = mnccl::ipc::liveness_queries();
  info->read_push = 1;  // since 6.0 the read schedule has only its push form
  info->auto_read = c->topology_allows_read() ? 1 : 0;
  for (int q = 0; q < 16; ++q) {
    info->peer_link[q] = q < c->nranks() ? c->peer_link(q) : -1;
    info->peer_hops[q] = q < c->nranks() ? c->peer_hops(q) : 0;
  }
  snprintf(info->auto_reason, sizeof info->auto_reason, "%s", c->topology_reason().c_str());
  info->read_grid_calls = c->read_grid_calls();
  info->window_calls = c->window_calls();
  info->windows = (int)c->windows();
  info->auto_grid = c->auto_grid() ? 1 : 0;
  info->retired_imports = (int)mnccl::ipc::retired_imports();
  info->retired_bytes = mnccl::ipc::retired_bytes();
  info->retired_budget = mnccl::ipc::retired_budget();
  info->budget_refusals = mnccl::ipc::budget_refusals();
  info->window_fast = c->window_fast() ? 1 : 0;
  info->run_pipelines = c->run_pipes();
  info->p2p_direct_recvs = c->p2p_direct_recvs();
  info->p2p_direct_sends = c->p2p_direct_sends();
  memcpy(out, &full, size < sizeof full ? size : sizeof full);
  return ncclSuccess;
}

// Collective in effect: every rank must select the same schedule before its next call (the
// schedules' messages share mailboxes and slots), as with any other communicator setting.
ncclResult_t mncclCommSetAlgo(ncclComm_t comm, int algo) {
  if (!comm) return ncclInvalidArgument;
  // mncclAlgoDirect (1) was removed in 400: it never beat the ring on any measured setup
  if (algo != mncclAlgoRing && algo != mncclAlgoRead && algo != mncclAlgoOneShot && algo != mncclAlgoReadGrid &&
      algo != mncclAlgoAuto)
    return ncclInvalidArgument;
  reinterpret_cast<Comm*>(comm)->set_algo(algo);
  return ncclSuccess;
}

ncclResult_t mncclCommLinkProbe(ncclComm_t comm, int allPeers, size_t bytes, int iters, double* gbps) {
  if (!comm || !gbps) return ncclInvalidArgument;
  try {
    return reinterpret_cast<Comm*>(comm)->link_probe(allPeers, bytes, iters, gbps);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] LinkProbe Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t mncclCommRegister(ncclComm_t comm, void* buff, size_t size, void** handle) {
  if (!comm || !buff || !handle || size == 0) return ncclInvalidArgument;
  try {
    return reinterpret_cast<Comm*>(comm)->register_window(buff, size, handle);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] CommRegister Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t mncclCommDeregister(ncclComm_t comm, void* handle) {
  if (!comm || !handle) return ncclInvalidArgument;
  try {
    return reinterpret_cast<Comm*>(comm)->deregister_window(handle);
  } catch (const std::exception& e) {
    fprintf(stderr, "[Mini-NCCL] CommDeregister Error: %s\n", e.what());
    return ncclInternalError;
  } catch (...) {
    return ncclSystemError;
  }
}

ncclResult_t mncclDataTypeSize(ncclDataType_t datatype, size_t* size) {
  if (!size || !dtype_ok(datatype)) return ncclInvalidArgument;
  *size = (size_t)mnccl::dtype_size((int)datatype);
  return ncclSuccess;
}

int mncclVersion(void) { return MNCCL_VERSION; }

}  // extern "C"
