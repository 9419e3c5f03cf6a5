// bootstrap.h -- TCP rendezvous for the communicator's one-time exchange.
//
// Plays the role of the reference's rank-0 star (RDMATransport.h:516-593 over
// Socket.h:31-107): rank 0 listens on ip:port, the others connect (bounded retries),
// and fixed-size records are all-gathered through rank 0.  The reference also ran
// this exchange on EVERY all-reduce (exchange_dynamic_info, RDMATransport.h:171-257);
// here it runs only in ncclCommInitRank / ncclCommDestroy: the hot path never touches
// the host network.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "split.h"

namespace mnccl {

class Bootstrap {
 public:
  Bootstrap() = default;
  ~Bootstrap();
  Bootstrap(const Bootstrap&) = delete;
  Bootstrap& operator=(const Bootstrap&) = delete;
  // a connected star changes hands (ncclCommSplit builds the child's star before the child)
  Bootstrap(Bootstrap&& o) noexcept;
  Bootstrap& operator=(Bootstrap&& o) noexcept;

  // Throws std::runtime_error on failure (bind/connect/timeout).
  void connect(int rank, int nranks, const std::string& ip, int port, double timeout_s);
  // connect()'s rank-0 half in two steps, "listen now, accept later": listen_on binds `port` (0: an
  // ephemeral one; loopback: 127.0.0.1 only) and returns the port it got; accept_members then makes
  // this object rank 0 of `nranks` once every other rank has connected.  A failure of either closes
  // the listening socket and every connection accepted so far.
  int listen_on(int port, bool loopback);
  void accept_members(int nranks, double timeout_s);
  // all-gather of `bytes` per rank: out receives nranks * bytes, rank-major
  void allgather(const void* mine, void* out, size_t bytes);
  void barrier();
  void close_all();

  int rank() const { return rank_; }
  int nranks() const { return nranks_; }

 private:
  static void send_all(int fd, const void* p, size_t n);
  static void recv_all(int fd, void* p, size_t n, double timeout_s);
  int rank_ = -1, nranks_ = 0;
  double timeout_s_ = 60.0;
  std::vector<int> clients_;  // rank 0: fd per rank (index = rank; [0] unused)
  int root_fd_ = -1;          // ranks > 0: connection to rank 0
  int listen_fd_ = -1;        // rank 0, between listen_on and accept_members
};

// The two rounds of ncclCommSplit over the parent's live star (collective over its ranks): every
// rank publishes (color, key) and computes the plan (split.h); then each group's leader, already
// listening on an ephemeral loopback port, publishes it and its members connect -- no well-known
// port, and the library is one-node.  Returns this rank's slot; `child` is then the group's
// connected star (untouched when the slot's size is 0, one rank without a socket when it is 1) and
// *port the leader's port (0 for a group of one or none).  Throws as connect does; `child` then
// holds no descriptor.
SplitSlot split_bootstrap(Bootstrap& parent, int color, int key, double timeout_s, Bootstrap* child, int* port);

}  // namespace mnccl
