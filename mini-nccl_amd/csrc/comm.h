// comm.h -- the communicator behind ncclComm_t (reference: Context + RDMATransport,
// include/mini_nccl.h:71-111 and src/transport/RDMATransport.h:99-637, re-designed for one
// MI355X node: HIP IPC over xGMI instead of verbs, device scratch instead of host-mapped).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "bootstrap.h"
#include "config.h"
#include "kernels.h"
#include "mini_nccl_api.h"
#include "p2p.h"
#include "peerbuf.h"
#include "schedule.h"

namespace mnccl {

class Comm {
 public:
  // Throws on failure; the API layer maps exceptions to ncclSystemError (api.cpp:62-65).
  Comm(int nranks, int rank, const std::string& ip);
  // What a communicator made by split() takes from its parent besides the Config: its sibling groups
  // run their persistent kernels on the same GPUs at the same time, so the residency cap
  // (exchange_and_map) is the family's, not the child's alone.  most: ranks on the most crowded GPU;
  // on_device: the divisor of the retired-import budget; run_pipes: the parent's run_pipes(), which
  // the child's never exceeds (0: no parent).  A child hands its own values on, so the root
  // ancestor's reach every descendant.
  struct Family {
    int most = 1, on_device = 1, run_pipes = 0;
  };
  // A child (ncclCommSplit): `boot` is its connected star (bootstrap.h split_bootstrap), `cfg` the
  // parent's Config by copy -- the environment is not read again -- and `board_port` its leader's
  // ephemeral port, which names the read schedule's board (peerbuf.cpp).  On the current device.
  Comm(Bootstrap&& boot, const Config& cfg, int board_port, const Family& fam);
  ~Comm();
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;

  // The hot path: returns an ncclResult_t; throws only on HIP runtime errors.
  // op: one of the four built-ins, or kPreMulSum with `scalar` the bits of the op's scalar (api.cpp
  // resolves a handle of redop_create before it calls; also reduce_scatter and reduce below)
  ncclResult_t allreduce(const void* send, void* recv, size_t count, int dtype, int op, hipStream_t stream,
                         uint64_t scalar = 0) {
    return collective(kCollAllReduce, send, recv, count, dtype, op, stream, 0, scalar);
  }
  // The all-reduce's two halves (NCCL's ncclReduceScatter / ncclAllGather; `count` per rank): send
  // holds n * count elements and recv gets chunk `rank` of their all-reduce, bit for bit; recv holds
  // n * count elements, rank q's send at [q * count, (q + 1) * count).  The read schedule
  // (kernels.hip scatter_fold / gather_push) where an all-reduce would run it, else the ring's
  // halves (schedule.h coll_op); no one-shot, no grid form, no registered windows.  In place as
  // NCCL defines it; any other overlap of the two buffers is ncclInvalidArgument.
  ncclResult_t reduce_scatter(const void* send, void* recv, size_t count, int dtype, int op, hipStream_t stream,
                              uint64_t scalar = 0) {
    return collective(kCollReduceScatter, send, recv, count, dtype, op, stream, 0, scalar);
  }
  ncclResult_t all_gather(const void* send, void* recv, size_t count, int dtype, hipStream_t stream) {
    return collective(kCollAllGather, send, recv, count, dtype, kSum, stream);
  }

  // The rooted collectives (NCCL's ncclBroadcast / ncclReduce over `count` elements): every rank's
  // recv gets the root's send; the root's recv gets the reduction of every rank's send, chunk c of
  // ceil(count / n) elements folded in the all-reduce's order for chunk c (no unreduced tail).  The
  // buffer a rank's role does not use (a non-root's send / recv) is ignored and may be NULL.  The
  // schedule choice is the halves': the read schedule (kernels.hip root_relay / root_fold), else
  // the ring (schedule.h coll_op).  root outside [0, n), a NULL buffer the role needs, or a partial
  // overlap on the root: ncclInvalidArgument, nothing launched or negotiated.
  ncclResult_t broadcast(const void* send, void* recv, size_t count, int dtype, int root, hipStream_t stream) {
    return collective(kCollBroadcast, send, recv, count, dtype, kSum, stream, root);
  }
  ncclResult_t reduce(const void* send, void* recv, size_t count, int dtype, int op, int root, hipStream_t stream,
                      uint64_t scalar = 0) {
    return collective(kCollReduce, send, recv, count, dtype, op, stream, root, scalar);
  }

  // User-created reduction ops (NCCL's ncclRedOpCreatePreMulSum / ncclRedOpDestroy): a handle is
  // kFirstUserOp + a slot of this communicator's table, at most kMaxUserOps live, a destroyed slot
  // handed out again.  A slot keeps the datatype the op was created for and the scalar's bits; a
  // call copies the bits into its kernel argument, so the op may be destroyed once the call is
  // issued.  redop_create: ncclInvalidUsage when the table is full.  redop_destroy: ncclInvalidArgument
  // for a built-in or unknown handle.  redop_find: false for an unknown handle.
  static constexpr int kFirstUserOp = 5, kMaxUserOps = 16;
  ncclResult_t redop_create(int* op, int dtype, uint64_t scalar);
  ncclResult_t redop_destroy(int op);
  bool redop_find(int op, int* dtype, uint64_t* scalar) const;
  ncclResult_t sticky_error() const { return sticky_; }

  // ncclCommSplit (mini_nccl_ext.h), after api.cpp's argument checks; collective over this
  // communicator's ranks.  Waits for the previous call, then two rounds over the bootstrap star
  // (split_bootstrap) and the child's construction on this communicator's device (the caller's is
  // restored).  *child: the new communicator, or nullptr for kSplitNoColor (ncclSuccess) and on any
  // failure: this communicator's sticky error, else ncclSystemError; this communicator stays usable.
  // The child is independent: own scratch, mailbox, counters, board, windows, user ops and star; it
  // may outlive this communicator.  Never throws.
  ncclResult_t split(int color, int key, Comm** child);

  // The all-to-all (RCCL's ncclAllToAll; `count` elements per block, n blocks in both buffers):
  // block q of this rank's send becomes block `rank` of rank q's recv, byte for byte.  The schedule
  // choice is the halves': the read schedule (kernels.hip exchange_push), else the ring (schedule.h
  // coll_op).  No in-place form: any overlap of the two buffers is ncclInvalidArgument, nothing
  // launched or negotiated.
  ncclResult_t all_to_all(const void* send, void* recv, size_t count, int dtype, hipStream_t stream) {
    return collective(kCollAllToAll, send, recv, count, dtype, kSum, stream);
  }

  // Gather and scatter (RCCL's ncclGather / ncclScatter; `count` elements per block): the root's
  // recv gets rank q's send as block q; rank q's recv gets block q of the root's send, byte for
  // byte.  The large buffer (Gather's recv, Scatter's send) is used on the root only: elsewhere it
  // is ignored and may be NULL.  The schedule choice is the halves': the read schedule (kernels.hip
  // collect_push / deal_push), else the ring (schedule.h coll_op).  In place on the root as NCCL
  // defines it; root outside [0, n), a NULL buffer the role needs, or any other overlap on the
  // root: ncclInvalidArgument, nothing launched or negotiated.
  ncclResult_t gather(const void* send, void* recv, size_t count, int dtype, int root, hipStream_t stream) {
    return collective(kCollGather, send, recv, count, dtype, kSum, stream, root);
  }
  ncclResult_t scatter(const void* send, void* recv, size_t count, int dtype, int root, hipStream_t stream) {
    return collective(kCollScatter, send, recv, count, dtype, kSum, stream, root);
  }

  // The variable all-to-all (RCCL's ncclAllToAllv; counts and displacements in elements, host arrays
  // of n entries read before the call returns): elements [sdispls[q], +sendcounts[q]) of this rank's
  // send become elements [rdispls[r], +recvcounts[r]) of rank q's recv.  A call path of its own
  // (comm.cpp): the local checks (varblock.h), a rendezvous that carries every rank's counts to every
  // rank whatever the schedule, then the read schedule (kernels.hip varblock_push) or, where the
  // rendezvous decides against it, the ring's all-to-all on blocks padded to the largest one.
  ncclResult_t all_to_all_v(const void* send, const size_t* sendcounts, const size_t* sdispls, void* recv,
                            const size_t* recvcounts, const size_t* rdispls, int dtype, hipStream_t stream);

  // The halves with per-rank counts (mncclAllGatherv / mncclReduceScatterv, mini_nccl_ext.h; counts and
  // displacements in elements, host arrays of n entries read before the call returns, the same on
  // every rank): rank q's send becomes elements [rdispls[q], +recvcounts[q]) of every rank's recv;
  // rank r's recv gets the reduction of elements [sdispls[r], +sendcounts[r]) of every rank's send in
  // the all-reduce's association for chunk r.  One call path for both (comm.cpp vhalf), modelled on
  // all_to_all_v: the local checks (vhalves.h), a rendezvous that carries every rank's arrays to every
  // rank and compares them for equality, then the read schedule (kernels.hip vhalf_push / vhalf_fold)
  // or, where the rendezvous decides against it, the ring's halves on blocks padded to the largest one.
  ncclResult_t all_gather_v(const void* send, size_t sendcount, void* recv, const size_t* recvcounts,
                            const size_t* rdispls, int dtype, hipStream_t stream) {
    return vhalf(kCollAllGatherV, recv, recvcounts, rdispls, const_cast<void*>(send), sendcount, dtype, kSum, stream, 0);
  }
  ncclResult_t reduce_scatter_v(const void* send, const size_t* sendcounts, const size_t* sdispls, void* recv,
                                size_t recvcount, int dtype, int op, hipStream_t stream, uint64_t scalar = 0) {
    return vhalf(kCollReduceScatterV, const_cast<void*>(send), sendcounts, sdispls, recv, recvcount, dtype, op, stream,
                 scalar);
  }

  // Point to point (NCCL's ncclSend / ncclRecv inside ncclGroupStart / ncclGroupEnd; api.cpp keeps
  // the group per thread, p2p.h its rules).  p2p_validate: one operation against the group recorded
  // so far -- the peer's range, the byte size, the overlaps (p2p.h p2p_check_op), then the buffer's
  // memory: device memory of this rank's GPU as is, pinned host memory through its device mapping
  // (reach), anything else ncclInvalidArgument -- and appends it; outside a group peer == rank is
  // ncclInvalidUsage.  p2p_group: every recorded operation as ONE launch of kernels.hip p2p_kernel on
  // the ring's scratch protocol, with no host rendezvous, between begin_call and end_call as any
  // collective; a self send or recv left unpaired, or paired with another size, is ncclInvalidUsage
  // with nothing launched.  last_algo reports the ring.
  // With at least one registered window (and more than one rank) the launch is kernels.hip
  // p2p_window_group instead: every recv whose range lies in a window with a table slot (p2p.h
  // p2p_win_direct) is posted direct and its sender pushes straight into it; the switch is
  // rank-uniform because registration is collective.  p2p_direct_recvs counts those recvs on the host;
  // p2p_direct_sends is the device's count of the messages this rank pushed direct, read from the
  // host-mapped control page (exact once the calls issued so far have completed).
  ncclResult_t p2p_validate(P2pGroup& g, bool grouped, bool send, int peer, const void* buf, size_t count, int dtype);
  ncclResult_t p2p_group(const P2pGroup& g, hipStream_t stream);
  // pipelines one point-to-point message may use (schedule.h p2p_pipes; the same on every rank)
  int p2p_pipes() const { return p2p_pipes_; }
  unsigned long long p2p_direct_recvs() const { return p2p_direct_recvs_; }
  unsigned long long p2p_direct_sends() const;

  int rank() const { return rank_; }
  int nranks() const { return nranks_; }
  int device() const { return device_; }
  const Config& config() const { return cfg_; }
  int algo() const { return auto_ ? -1 : algo_; }
  // a < 0: the default (read for buffers every rank can share; for the other calls the one-shot
  // when small, else the ring); 0 ring, 2 read, 3 one-shot wherever a call fits it, 4 read with
  // its large calls in the grid form (kernels.hip read_grid_kernel)
  void set_algo(int a) {
    auto_ = a < 0;
    algo_ = a < 0 ? 2 : a;
  }
  int last_algo() const { return last_algo_; }  // schedule of the last launched kernel, -1: none
  // Registered windows (mncclCommRegister / mncclCommDeregister, collective): a call whose send and
  // recv lie in windows -- the same windows at the same offsets on every rank -- runs the read
  // schedule with no host rendezvous (kernels.hip starts_agree checks the promise on the device)
  ncclResult_t register_window(void* buf, size_t bytes, void** handle);
  ncclResult_t deregister_window(void* handle);
  size_t windows() const { return windows_.size(); }
  unsigned long long window_calls() const { return window_calls_; }
  bool window_fast() const { return window_fast_; }  // window calls skip the host rendezvous
  unsigned long long read_grid_calls() const { return read_grid_calls_; }  // calls run in the grid form
  size_t peer_mappings() const { return pbuf_.mapped_allocations(); }
  const PeerBuffers& peer_buffers() const { return pbuf_; }
  // rank processes / communicators whose GPU is this rank's GPU (this rank included)
  int ranks_on_device() const { return ranks_on_device_; }
  // auto's topology rule (schedule.h topology_blocks_read), the same on every rank: whether the
  // default runs the read schedule, why, and how this rank's GPU reaches each peer's
  bool topology_allows_read() const { return topo_read_; }
  bool auto_grid() const { return auto_ && topo_read_; }  // auto's large read calls: grid form
  const std::string& topology_reason() const { return topo_why_; }
  int peer_link(int q) const { return peer_link_[q]; }
  int peer_hops(int q) const { return peer_hops_[q]; }
  ncclResult_t async_error();
  // Collective: every rank writes `bytes` into the next rank's scratch (all_peers = 0) or into
  // every peer's scratch at once (1), `iters` times; *gbps = bytes per second per link
  // direction (max over nothing: this rank's own time).  No all-reduce may be in flight.
  ncclResult_t link_probe(int all_peers, size_t bytes, int iters, double* gbps);
  size_t scratch_bytes() const { return scratch_bytes_; }
  // kernel geometry (schedule.h pipeline_geometry): one pipeline per wave, each moving up to
  // slot_bytes (MINI_NCCL_SLICE_SIZE unless the scratch cap shrank it) per message
  int workgroups() const { return geo_.workgroups; }
  int wave_channels() const { return geo_.workgroups * geo_.waves; }
  // the pipelines a call may launch: wave_channels(), capped so that every co-located rank's waves
  // fit the GPU at once (exchange_and_map)
  int run_pipes() const { return run_pipes_ > 0 ? run_pipes_ : wave_channels(); }
  uint64_t wave_slice() const { return geo_.slot_bytes; }

 private:
  void setup_device_resources();
  void release();
  void exchange_and_map();
  void classify_topology(const void* records);  // records: every rank's init record (comm.cpp)
  ncclResult_t wait_for(hipStream_t stream, uint32_t seq);
  enum class Reach { kDevice, kMapped, kStaged };
  Reach reach(const void* p, const void** kernel_ptr, bool* local) const;
  void ensure_stage(size_t bytes, hipStream_t stream);
  // algo: 0 ring, 2 read (psend / precv: every rank's buffers mapped here), 3 one-shot
  // coll (schedule.h Coll): a reduce-scatter's recv and an all-gather's send hold one chunk; the
  // kernels get them shifted by rank * chunk_bytes and keep the all-reduce's index math
  void launch(int algo, const void* send, void* recv, size_t chunk_bytes, int dtype, int op, hipStream_t stream,
              uint32_t seq, bool vec, const char* const* psend = nullptr, const char* const* precv = nullptr,
              size_t tail_bytes = 0, uint64_t sig = 0, int coll = kCollAllReduce, int root = 0,
              size_t total_bytes = 0, uint64_t scalar = 0);
  CollParams make_params(int algo, const void* send, void* recv, size_t chunk_bytes, uint32_t seq,
                         const char* const* psend, const char* const* precv, size_t tail_bytes, uint64_t sig, int coll,
                         int root, size_t total_bytes, int* pipes);
  // what every call does around its work (collective() and all_to_all_v()): this rank's device made
  // current, the stream's capture state, the order after the communicator's previous call; then the
  // order event, the caller's device restored and the blocking mode's wait
  struct CallScope {
    int cur_dev = -1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    bool capturing() const { return cap != hipStreamCaptureStatusNone; }
  };
  CallScope begin_call(hipStream_t stream);
  ncclResult_t end_call(const CallScope& sc, hipStream_t stream, uint32_t seq);
  // every rank's ncclAllToAllv row where the board is unavailable: over the bootstrap, like
  // mncclCommLinkProbe's records.  False: the ranks disagree on the collective or the datatype
  // (mncclAllGatherv / mncclReduceScatterv pass their collective, op and scalar bits: compared too)
  bool gather_rows(const VarRow& mine, int dtype, VarRow* rows, int coll = kCollAllToAllV, int op = 0,
                   uint64_t scalar = 0);
  // mncclAllGatherv / mncclReduceScatterv: array_buf / counts / displs the side with n blocks (the
  // gather's recv, the scatter's send), one_buf / one_count this rank's one block
  ncclResult_t vhalf(int coll, void* array_buf, const size_t* counts, const size_t* displs, void* one_buf,
                     size_t one_count, int dtype, int op, hipStream_t stream, uint64_t scalar);
  // the one call path of the eight collectives; count: the all-reduce's and the rooted ones', per
  // rank for the halves, per block for the all-to-all, the gather and the scatter
  ncclResult_t collective(int coll, const void* send, void* recv, size_t count, int dtype, int op,
                          hipStream_t stream, int root = 0, uint64_t scalar = 0);
  // a kPreMulSum call on a communicator of one rank: recv = round(scalar * send) over `count` elements
  void scale_one_rank(const void* send, void* recv, size_t count, int dtype, uint64_t scalar, const CallScope& sc,
                      hipStream_t stream);
  // one rendezvous failure of the read schedule, reported like the kernel's (sticky, peers aborted)
  ncclResult_t rendezvous_failed(const std::exception& e, bool peer_gave_up, int cur_dev);
  struct Window {
    uint64_t id;                    // registration number, the same on every rank
    const char* base;               // this rank's buffer
    size_t bytes;
    const char* peer[kMaxRanks];    // every rank's buffer of this window, mapped here
    bool aligned;                   // every rank's base is dword-aligned
    int slot;                       // its slot of the point-to-point window table (p2p.h), -1: none
  };
  void upload_win_table();          // win_host_ -> win_table_, after wait_previous_call
  const Window* find_window(const void* p, size_t bytes) const;
  void wait_previous_call();
  ncclResult_t check_status();
  // a rank that gives up on a call outside its kernel (the read schedule's rendezvous) raises
  // every peer's ABORT word, as a timed-out kernel does, so the peers fail fast instead of
  // running into their own watchdog
  void abort_peers();

  int rank_, nranks_, device_ = 0;
  Config cfg_;
  Family fam_;                   // a child's inheritance (split); a root communicator's defaults
  int most_ = 1, budget_div_ = 1;  // what this communicator's own children inherit (exchange_and_map)
  int board_port_ = 0;           // names the read schedule's board: MINI_NCCL_PORT, a child's leader's port
  Geometry geo_;
  int algo_ = 0;                 // 0 ring, 2 read (its calls fall back to the ring when some rank's
                                 // buffers cannot be shared), 3 one-shot (larger calls: as auto)
  bool auto_ = true;             // the default: as algo_ = 2, with the ring's small calls one-shot
  int last_algo_ = -1;
  unsigned long long read_grid_calls_ = 0;  // read calls launched as start / grid / done
  std::vector<Window> windows_;
  uint64_t next_window_ = 1;
  unsigned long long window_calls_ = 0;     // calls launched on registered windows (no rendezvous)
  bool window_fast_ = true;                 // window calls skip the host rendezvous (MINI_NCCL_WINDOW_RENDEZVOUS)
  int run_pipes_ = 0;                       // 0 until exchange_and_map: run_pipes()
  int ranks_on_device_ = 1;
  int p2p_pipes_ = 1;                       // schedule.h p2p_pipes (exchange_and_map)
  P2pWinSlots win_slots_;                   // which window holds which slot of the table below
  P2pWinTable win_host_;                    // the host's copy of base / bytes (upload_win_table)
  P2pWinTable* win_table_ = nullptr;        // device: the table p2p_window_group reads (nranks > 1)
  unsigned long long p2p_direct_recvs_ = 0; // recv operations posted direct
  bool topo_read_ = true;        // auto may run the read schedule (every pair: same GPU or 1 xGMI hop)
  std::string topo_why_ = "read: one rank";
  int peer_link_[kMaxRanks] = {}, peer_hops_[kMaxRanks] = {};
  uint32_t call_seq_ = 0;        // kernel launches of this communicator (the kernel's start word)
  Bootstrap boot_;

  char* scratch_ = nullptr;      // uncached device memory, peers write into it
  size_t scratch_bytes_ = 0;
  uint64_t* mbox_ = nullptr;     // uncached device memory: READY / CREDIT / ABORT words
  size_t mbox_bytes_ = 0;
  uint64_t* pair_seq_ = nullptr; // [2][n][C]: per (peer, channel) tx / rx message counters (device)
  uint32_t* claim_ = nullptr;    // after them: the kernels' first-give-up word (kernels.h)
  uint32_t* go_ = nullptr;       // and the grid form's START-through word (kernels.h CollParams::go)
  uint32_t* h_ctl_ = nullptr;    // host-mapped: [0] status, [1] abort request, [2] last started call
  uint32_t* d_ctl_ = nullptr;    // device view of h_ctl_

  std::vector<char*> peer_scratch_;
  std::vector<uint64_t*> peer_mbox_;
  hipIpcMemHandle_t scratch_h_, mbox_h_;  // exported once (pool blocks, ipcreg.h)
  uint64_t scratch_id_ = 0, mbox_id_ = 0;
  PeerBuffers pbuf_;               // read schedule: per-call rendezvous + peers' buffer mappings
  std::vector<uint64_t> owners_;   // process nonces of the peers in other processes
  bool registered_ = false;        // ipc::comm_opened(owners_) done

  char* stage_ = nullptr;         // device staging copy for pageable host buffers (grown on demand)
  size_t stage_bytes_ = 0;
  char* var_stub_ = nullptr;      // ncclAllToAllv (and the halves with per-rank counts): stands in for a rank's NULL buffers in the rendezvous
                                  // (an idle rank passes none); allocated on first need

  hipEvent_t order_ev_ = nullptr;     // recorded after every call: cross-stream ordering, and the
                                      // blocking call's completion (wait_for)
  hipStream_t last_stream_ = nullptr;
  bool have_last_ = false;
  ncclResult_t sticky_ = ncclSuccess;
  bool warned_capture_ = false;
  struct UserOp {
    bool live = false;
    int dtype = 0;
    uint64_t scalar = 0;
  };
  UserOp user_ops_[kMaxUserOps];
};

// 1-GPU local reduce (mini_nccl_ext.h): no communicator needed.
ncclResult_t local_reduce(void* out, const void* local, const void* incoming, size_t count, int dtype, int op,
                          hipStream_t stream);

}  // namespace mnccl
