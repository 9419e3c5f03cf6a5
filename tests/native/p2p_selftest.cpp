// p2p_selftest.cpp -- csrc/p2p.h (the bookkeeping of ncclSend / ncclRecv groups) and the
// point-to-point geometry of csrc/schedule.h as a stand-alone program: overlap detection, the
// size_t overflow, kMaxGroupOps, self pairing (equal, unequal, unpaired), per-pair ordering and the
// launch's wave mapping.  tests/test_p2p_cpu.py builds and runs it twice, plain and with
// -fsanitize=address,undefined; it is never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "p2p.h"

using namespace mnccl;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// check + append, as Comm::p2p_validate does on a buffer the kernel can address as is
static int add(P2pGroup& g, int n, bool send, int peer, uint64_t addr, size_t count, int esz) {
  uint64_t bytes = 0;
  const int v = p2p_check_op(g, n, send, peer, (const void*)(uintptr_t)addr, count, esz, &bytes);
  if (v != kP2pOk) return v;
  return p2p_append(g, send, peer, (const void*)(uintptr_t)addr, addr, bytes);
}

static void test_checks() {
  const uint64_t top = ~(uint64_t)0;
  P2pGroup g;
  // the peer's range, before anything else
  CHECK(add(g, 4, true, -1, 0x1000, 4, 4) == kP2pPeerRange);
  CHECK(add(g, 4, true, 4, 0x1000, 4, 4) == kP2pPeerRange);
  CHECK(add(g, 4, false, 4, 0x1000, (size_t)top, 8) == kP2pPeerRange);
  // overflow: the byte size, the buffer's end
  CHECK(add(g, 4, true, 1, 0x1000, (size_t)(top / 4 + 1), 4) == kP2pOverflow);
  CHECK(add(g, 4, true, 1, 0x1000, (size_t)top, 2) == kP2pOverflow);
  CHECK(add(g, 4, false, 1, top - 15, 2, 8) == kP2pOverflow);
  CHECK(add(g, 4, false, 1, top - 16, 2, 8) == kP2pOk);  // ends at the last byte
  CHECK(g.nops == 1);
  // overlaps: sends may overlap sends; a recv overlaps nothing
  P2pGroup h;
  CHECK(add(h, 4, true, 1, 0x1000, 16, 4) == kP2pOk);   // send [0x1000, 0x1040)
  CHECK(add(h, 4, true, 2, 0x1020, 16, 4) == kP2pOk);   // send overlapping a send: only read
  CHECK(add(h, 4, true, 2, 0x1000, 16, 4) == kP2pOk);   // the same buffer to another peer
  CHECK(add(h, 4, false, 1, 0x103c, 4, 4) == kP2pOverlap);  // recv over a send's last element
  CHECK(add(h, 4, false, 1, 0x105f, 1, 2) == kP2pOverlap);  // one byte into the second send
  CHECK(add(h, 4, false, 1, 0x1060, 4, 4) == kP2pOk);       // adjacent: recv [0x1060, 0x1070)
  CHECK(add(h, 4, false, 3, 0x106c, 1, 4) == kP2pOverlap);  // recv over a recv
  CHECK(add(h, 4, false, 3, 0x1070, 1, 4) == kP2pOk);
  CHECK(add(h, 4, true, 3, 0x1068, 4, 4) == kP2pOverlap);   // a later send over a recv
  CHECK(add(h, 4, true, 3, 0x0ff0, 4, 4) == kP2pOk);        // ends where the first send starts
  CHECK(h.nops == 6);
  // kMaxGroupOps
  P2pGroup m;
  for (int i = 0; i < kMaxGroupOps; ++i) CHECK(add(m, 2, i % 2 == 0, 1, 0x10000 + 64 * (uint64_t)i, 8, 4) == kP2pOk);
  CHECK(add(m, 2, true, 1, 0x90000, 8, 4) == kP2pTooMany);
  CHECK(m.nops == kMaxGroupOps);
  P2pArgs a;
  CHECK(p2p_build(m, 0, 4, 1024, &a) == kP2pOk);
  CHECK(a.npairs == 2 && a.pair_count[0] == kMaxGroupOps / 2 && a.pair_count[1] == kMaxGroupOps / 2 && a.nself == 0);
  CHECK(sizeof(P2pArgs) <= 2048);  // with CollParams inside a by-value kernel argument block
}

static void test_self_pairing() {
  P2pArgs a;
  {  // equal sizes pair in order: the k-th send with the k-th recv
    P2pGroup g;
    CHECK(add(g, 3, true, 1, 0x1000, 8, 4) == kP2pOk);
    CHECK(add(g, 3, false, 1, 0x2000, 5, 4) == kP2pOk);   // self recv first
    CHECK(add(g, 3, true, 1, 0x3000, 5, 4) == kP2pOk);    // pairs with it
    CHECK(add(g, 3, true, 1, 0x4000, 300, 2) == kP2pOk);  // second self send ...
    CHECK(add(g, 3, false, 1, 0x5002, 150, 4) == kP2pOk); // ... second self recv: same bytes, other datatype
    g.ops[0].peer = 2;  // (the first operation goes to a peer)
    CHECK(p2p_build(g, 1, 4, 1024, &a) == kP2pOk);
    CHECK(a.npairs == 1 && a.pair_peer[0] == 2 && a.pair_send[0] == 1 && a.pair_count[0] == 1 && a.pipes == 1);
    CHECK(a.nself == 2 && a.self_first == 1 && a.self_waves == 1);
    CHECK(a.ptr[1] == 0x3000 && a.ptr[2] == 0x2000 && a.bytes[1] == 20 && a.bytes[2] == 20 && a.vec[1] == 1);
    CHECK(a.ptr[3] == 0x4000 && a.ptr[4] == 0x5002 && a.bytes[3] == 600 && a.vec[3] == 0 && a.vec[4] == 0);
    CHECK(p2p_launch_waves(a) == 2);
  }
  {  // unequal bytes
    P2pGroup g;
    CHECK(add(g, 2, true, 0, 0x1000, 8, 4) == kP2pOk);
    CHECK(add(g, 2, false, 0, 0x2000, 8, 2) == kP2pOk);
    CHECK(p2p_build(g, 0, 4, 1024, &a) == kP2pSelfSize);
  }
  {  // unpaired: a send alone, a recv alone, two sends and one recv
    P2pGroup g;
    CHECK(add(g, 2, true, 0, 0x1000, 8, 4) == kP2pOk);
    CHECK(p2p_build(g, 0, 4, 1024, &a) == kP2pSelfUnpaired);
    CHECK(p2p_build(g, 1, 4, 1024, &a) == kP2pOk);  // seen from rank 1 it is a send to a peer
    CHECK(add(g, 2, false, 0, 0x2000, 8, 4) == kP2pOk);
    CHECK(p2p_build(g, 0, 4, 1024, &a) == kP2pOk);
    CHECK(add(g, 2, true, 0, 0x3000, 8, 4) == kP2pOk);
    CHECK(p2p_build(g, 0, 4, 1024, &a) == kP2pSelfUnpaired);
    P2pGroup h;
    CHECK(add(h, 1, false, 0, 0x2000, 8, 4) == kP2pOk);
    CHECK(p2p_build(h, 0, 1, 1024, &a) == kP2pSelfUnpaired);
  }
  {  // one rank: the self pair alone, its waves by size
    P2pGroup g;
    CHECK(add(g, 1, true, 0, 0x100000, 1 << 20, 4) == kP2pOk);
    CHECK(add(g, 1, false, 0, 0x900000, 1 << 20, 4) == kP2pOk);
    CHECK(p2p_build(g, 0, 1, 1024, &a) == kP2pOk);
    CHECK(a.npairs == 0 && a.pipes == 0 && a.nself == 1 && a.self_waves == kP2pMaxSelfWaves);
    CHECK(p2p_launch_waves(a) == kP2pMaxSelfWaves);
  }
  {  // an empty group launches nothing
    P2pGroup g;
    CHECK(p2p_build(g, 0, 4, 1024, &a) == kP2pOk && p2p_launch_waves(a) == 0);
  }
}

static void test_pair_ordering() {
  // rank 1 of 4: operations of several pairs interleaved; pairs in order of first appearance, a
  // pair's operations in call order, the launch as wide as its widest message
  P2pGroup g;
  const uint64_t slot = 1024;
  struct { bool send; int peer; uint64_t addr; size_t bytes; } ops[] = {
      {true, 2, 0x10000, 100},        // pair 0 = (send, 2)
      {false, 0, 0x20002, 5000},      // pair 1 = (recv, 0): 5 slices, odd alignment
      {true, 2, 0x30000, 3 * 1024},   // pair 0 again: 3 slices
      {true, 0, 0x40000, 1024},       // pair 2 = (send, 0): a send to the peer it also receives from
      {false, 0, 0x50000, 2},         // pair 1 again
      {false, 3, 0x60000, 64 * 1024}, // pair 3 = (recv, 3): 64 slices, capped at the 4 pipelines
      {true, 2, 0x70000, 1},          // pair 0, third
  };
  for (auto& o : ops) CHECK(add(g, 4, o.send, o.peer, o.addr, o.bytes, 1) == kP2pOk);
  P2pArgs a;
  CHECK(p2p_build(g, 1, 4, slot, &a) == kP2pOk);
  CHECK(a.npairs == 4 && a.pipes == 4 && a.p2p_pipes == 4 && a.nself == 0 && a.self_waves == 0 && a.self_first == 7);
  const int want_peer[4] = {2, 0, 0, 3}, want_send[4] = {1, 0, 1, 0}, want_first[4] = {0, 3, 5, 6}, want_count[4] = {3, 2, 1, 1};
  for (int p = 0; p < 4; ++p)
    CHECK(a.pair_peer[p] == want_peer[p] && a.pair_send[p] == want_send[p] && a.pair_first[p] == want_first[p] &&
          a.pair_count[p] == want_count[p]);
  const uint64_t want_ptr[7] = {0x10000, 0x30000, 0x70000, 0x20002, 0x50000, 0x40000, 0x60000};
  const uint64_t want_bytes[7] = {100, 3072, 1, 5000, 2, 1024, 65536};
  const int want_vec[7] = {1, 1, 1, 0, 1, 1, 1};
  for (int i = 0; i < 7; ++i) CHECK(a.ptr[i] == want_ptr[i] && a.bytes[i] == want_bytes[i] && a.vec[i] == want_vec[i]);
  CHECK(p2p_launch_waves(a) == 16);
  // the same group on fewer pipelines per message is narrower
  CHECK(p2p_build(g, 1, 2, slot, &a) == kP2pOk && a.pipes == 2 && p2p_launch_waves(a) == 8);
}

static void test_geometry() {
  // a message's slices and pipelines from its bytes alone; every slice on exactly one pipeline
  for (uint64_t slot : {(uint64_t)1024, (uint64_t)4096})
    for (int pipes : {1, 2, 3, 8})
      for (uint64_t bytes : {(uint64_t)1, slot - 1, slot, slot + 1, 2 * slot, 2 * slot * pipes, 6 * slot * pipes + 20}) {
        const uint64_t ns = p2p_nslices(bytes, slot);
        const int A = p2p_msg_pipes(bytes, slot, pipes);
        CHECK(A >= 1 && A <= pipes && (uint64_t)A <= ns);
        uint64_t msgs = 0, total = 0;
        for (int w = 0; w < pipes; ++w) {
          uint64_t mine = 0;
          for (uint64_t s = (uint64_t)w; w < A && s < ns; s += (uint64_t)A) {
            ++mine;
            total += slice_len(bytes, slot, s);
          }
          CHECK(p2p_pipe_msgs(bytes, slot, pipes, w) == mine);
          msgs += mine;
        }
        CHECK(msgs == ns && total == bytes);
      }
  // p2p_pipes: at least 1, at most C, pairs x pipes inside the resident budget
  for (int n : {1, 2, 3, 8, 16})
    for (int C : {1, 2, 256})
      for (int most : {1, 8, 16}) {
        const int p = p2p_pipes(n, C, 256, most, 2), cap = resident_cap(1, 256, most, 2);
        CHECK(p >= 1 && p <= C);
        if (n > 1) CHECK(2 * (n - 1) * p <= cap);
        CHECK(resident_pipes(C, 1, 256, most, 2) == (C < cap ? C : cap));
      }
  CHECK(p2p_pipes(2, 256, 256, 2, 2) == 256 && p2p_pipes(4, 256, 256, 4, 2) == 85 && p2p_pipes(16, 256, 256, 16, 2) == 4);
}

int main() {
  test_checks();
  test_self_pairing();
  test_pair_ordering();
  test_geometry();
  if (failures) {
    fprintf(stderr, "p2p selftest: %d failure(s)\n", failures);
    return 1;
  }
  printf("p2p selftest: ok\n");
  return 0;
}
