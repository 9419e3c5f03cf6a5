// alltoallv_selftest.cpp -- ncclAllToAllv's host side under AddressSanitizer +
// UndefinedBehaviorSanitizer, run by tests/test_alltoallv_cpu.py.  A stand-alone program:
//  * the simulator (csrc/sim.cpp mnccl_sim_varblock: the mirror of kernels.hip varblock_push on the
//    read schedule, the padded ring otherwise) on a handful of the CPU suite's cases -- random bytes
//    in, the permutation out, gaps and guard bytes unchanged;
//  * the local and matrix checks (csrc/varblock.h) on hand-made cases;
//  * the board's rendezvous with rows (csrc/peerbuf.cpp, set_test_fake: no GPU), one thread per
//    rank: every rank gets the same matrix, the mismatch verdict and the capture-flag verdict.
// Exits non-zero on any failure.  argv[1]: the TCP port of the bootstrap (default: from the pid).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <thread>
#include <vector>

#include "bootstrap.h"
#include "peerbuf.h"
#include "varblock.h"

extern "C" int mnccl_sim_varblock(int n, int calls, const int* coll, const int* sched, const uint64_t* counts,
                                  const int* roots, const float* const* send, float* const* recv, int esz,
                                  const uint64_t* vcounts, const uint64_t* vsdispls, const uint64_t* vrdispls, int op,
                                  uint64_t slice_bytes, uint64_t min_slice, int channels, int slots,
                                  uint64_t schedule_seed, uint64_t* steps_out);

namespace {

constexpr size_t kGuard = 256;
constexpr unsigned char kFill = 0xA5;

uint64_t next(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// mode 0 contiguous, 1 reversed, 2 reversed with 3-element gaps; returns the length in elements
uint64_t layout(const std::vector<uint64_t>& counts, int mode, std::vector<uint64_t>& displs) {
  const int n = (int)counts.size();
  const uint64_t gap = mode == 2 ? 3 : 0;
  uint64_t at = gap;
  displs.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const int q = mode == 0 ? i : n - 1 - i;
    displs[(size_t)q] = at;
    at += counts[(size_t)q] + gap;
  }
  return at ? at : 1;
}

// `scheds.size()` variable all-to-alls on one state, the matrix drawn from `values` (kind 0), all
// zero (1), one large block among empty ones (2), or with a zero row and column (3)
int run_case(int n, int esz, int kind, int mode, uint64_t slice, int channels, const std::vector<int>& scheds, uint64_t seed) {
  const uint64_t values[] = {0, 1, 3, 300, 16411 / 8};
  const size_t k = scheds.size(), nn = (size_t)n * n;
  uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 1;
  std::vector<uint64_t> vc(k * nn), vs(k * nn), vr(k * nn), counts(k, 0);
  std::vector<int> coll(k, 6), roots(k, 0);
  std::vector<std::vector<float>> send(k * n), recv(k * n);
  std::vector<size_t> rbytes(k * n);
  std::vector<const float*> sp(k * n);
  std::vector<float*> rp(k * n);
  for (size_t i = 0; i < k; ++i) {
    uint64_t* C = &vc[i * nn];
    for (int r = 0; r < n; ++r)
      for (int q = 0; q < n; ++q) {
        uint64_t c = values[next(rng) % 5];
        if (kind == 1) c = 0;
        if (kind == 2) c = r == n - 1 && q == 0 ? 5000 : 0;
        if (kind == 3 && (r == 0 || q == 0)) c = 0;
        C[(size_t)r * n + q] = c;
      }
    for (int r = 0; r < n; ++r) {
      std::vector<uint64_t> sc((size_t)n), rc((size_t)n), d;
      for (int q = 0; q < n; ++q) sc[(size_t)q] = C[(size_t)r * n + q], rc[(size_t)q] = C[(size_t)q * n + r];
      const size_t sb = (size_t)layout(sc, mode, d) * esz;
      for (int q = 0; q < n; ++q) vs[i * nn + (size_t)r * n + q] = d[(size_t)q];
      const size_t rb = (size_t)layout(rc, mode, d) * esz;
      for (int q = 0; q < n; ++q) vr[i * nn + (size_t)r * n + q] = d[(size_t)q];
      std::vector<float>& s = send[i * n + r];
      std::vector<float>& t = recv[i * n + r];
      s.resize(sb / 4 + 1);
      for (size_t b = 0; b < sb; ++b) ((unsigned char*)s.data())[b] = (unsigned char)next(rng);
      t.resize((rb + kGuard) / 4 + 1);
      memset(t.data(), kFill, t.size() * 4);
      rbytes[i * n + r] = rb;
      sp[i * n + r] = s.data();
      rp[i * n + r] = t.data();
    }
  }
  const std::vector<std::vector<float>> before = send;
  uint64_t steps = 0;
  const int rc = mnccl_sim_varblock(n, (int)k, coll.data(), scheds.data(), counts.data(), roots.data(), sp.data(), rp.data(),
                                    esz, vc.data(), vs.data(), vr.data(), 0, slice, 0, channels, 2, seed, &steps);
  if (rc != 0) {
    fprintf(stderr, "n=%d kind=%d mode=%d slice=%llu: rc %d\n", n, kind, mode, (unsigned long long)slice, rc);
    return 1;
  }
  for (size_t i = 0; i < k; ++i)
    for (int q = 0; q < n; ++q) {
      // the expected recv: the fill, with the block from every rank r at rank q's rdispls[r]
      std::vector<unsigned char> exp(rbytes[i * n + q] + kGuard, kFill);
      for (int r = 0; r < n; ++r) {
        const uint64_t c = vc[i * nn + (size_t)r * n + q] * esz;
        memcpy(exp.data() + vr[i * nn + (size_t)q * n + r] * esz,
               (const unsigned char*)before[i * n + r].data() + vs[i * nn + (size_t)r * n + q] * esz, (size_t)c);
      }
      if (memcmp(recv[i * n + q].data(), exp.data(), exp.size()) != 0) {
        fprintf(stderr, "n=%d kind=%d mode=%d slice=%llu call %zu: rank %d's recv (blocks, gaps or guard) differs\n", n,
                kind, mode, (unsigned long long)slice, i, q);
        return 1;
      }
      if (memcmp(send[i * n + q].data(), before[i * n + q].data(), send[i * n + q].size() * 4) != 0) {
        fprintf(stderr, "n=%d call %zu: rank %d's send was written\n", n, i, q);
        return 1;
      }
    }
  return 0;
}

int expect(bool ok, const char* what) {
  if (!ok) fprintf(stderr, "check failed: %s\n", what);
  return ok ? 0 : 1;
}

int check_rules() {
  using namespace mnccl;
  int bad = 0;
  const void* s = (const void*)(uintptr_t)0x10000;
  const void* r = (const void*)(uintptr_t)0x80000;
  const size_t c3[3] = {4, 0, 7}, d3[3] = {0, 4, 4}, z3[3] = {0, 0, 0};
  bad += expect(varblock_check_local(3, 4, s, c3, d3, r, c3, d3) == kVarOk, "a valid call");
  bad += expect(varblock_check_local(3, 4, nullptr, z3, z3, nullptr, z3, z3) == kVarOk, "NULL buffers with zero counts");
  bad += expect(varblock_check_local(3, 4, nullptr, c3, d3, r, c3, d3) == kVarNullBuffer, "NULL send with counts");
  bad += expect(varblock_check_local(3, 4, s, z3, z3, nullptr, c3, d3) == kVarNullBuffer, "NULL recv with counts");
  const size_t over[3] = {0, 3, 3};  // block 2 starts inside block 0
  bad += expect(varblock_check_local(3, 4, s, c3, d3, r, c3, over) == kVarRecvOverlap, "overlapping recv blocks");
  bad += expect(varblock_check_local(3, 4, s, c3, over, r, c3, d3) == kVarOk, "overlapping send blocks are accepted");
  bad += expect(varblock_check_local(3, 4, s, c3, d3, (const char*)s + 40, c3, d3) == kVarSendRecvOverlap,
                "recv overlaps send");
  const size_t huge[3] = {~(size_t)0 - 2, 0, 0};
  bad += expect(varblock_check_local(3, 4, s, c3, huge, r, c3, d3) == kVarOverflow, "displ + count overflows");
  const size_t big[3] = {~(size_t)0 / 4 + 1, 0, 0};
  bad += expect(varblock_check_local(3, 4, s, big, z3, r, c3, d3) == kVarOverflow, "byte size overflows");
  VarRow rows[3];
  memset(rows, 0, sizeof rows);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) rows[a].sendcounts[b] = rows[b].recvcounts[a] = (uint64_t)(a * 3 + b);
  bad += expect(varblock_matrix_mismatch(3, rows) == 0, "a consistent matrix");
  bad += expect(varblock_max_count(3, rows) == 8, "the largest block");
  rows[2].recvcounts[1] += 1;
  bad += expect(varblock_matrix_mismatch(3, rows) == 1 + 1 * 3 + 2, "a one-element mismatch");
  bad += expect(!varblock_any_capturing(3, rows), "no rank capturing");
  rows[1].flags = kVarCapturing;
  bad += expect(varblock_any_capturing(3, rows), "a rank capturing");
  return bad;
}

// The rendezvous with rows: n rank threads on one board, synthetic buffers (set_test_fake)
struct BoardOut {
  int decisions[5];
  mnccl::VarRow rows[5][mnccl::kVarMaxRanks];
  bool capture[5];
  bool threw = false;
};

void board_rank(int rank, int n, int port, BoardOut* out) {
  using namespace mnccl;
  try {
    Bootstrap b;
    b.connect(rank, n, "127.0.0.1", port, 20.0);
    std::vector<uint64_t> nonces((size_t)n);
    for (int q = 0; q < n; ++q) nonces[(size_t)q] = 7000u + (uint64_t)q;  // "one process per rank"
    PeerBuffers pb;
    pb.set_test_fake(true, 0);
    pb.init(b, rank, n, nonces, port);
    if (!pb.available()) {
      out->threw = true;
      b.barrier();
      return;
    }
    std::vector<char> arena(64 << 10);
    const int form = 0xff | 6 << 8;
    for (int call = 0; call < 5; ++call) {
      VarRow mine;
      memset(&mine, 0, sizeof mine);
      for (int q = 0; q < n; ++q) {
        mine.sendcounts[q] = (uint64_t)(100 * call + 10 * rank + q);  // C[r][q]
        mine.recvcounts[q] = (uint64_t)(100 * call + 10 * q + rank);  // C[q][r]
        mine.rdispls[q] = (uint64_t)(1000 * rank + q);
      }
      if (call == 1 && rank == n - 1) mine.recvcounts[0] += 1;  // a one-element mismatch
      if (call == 2 && rank == 1) mine.flags = kVarCapturing;
      const bool eligible = !((call == 2 || call == 3) && rank == 0);  // calls 2 and 3: the fallback
      const char* ps[kVarMaxRanks] = {};
      const char* pr[kVarMaxRanks] = {};
      bool vec = false;
      const void* sb = arena.data() + (size_t)(2 * (call % 2)) * 4096;
      const void* rb = arena.data() + (size_t)(2 * (call % 2) + 1) * 4096;
      if (call == 4) {  // a call that passes no row, between the others: the scalar count as before
        out->decisions[call] = (int)pb.negotiate(sb, rb, true, 1234, 7, 0, 20.0, [] {}, ps, pr, &vec, 0xff | 5 << 8);
        out->capture[call] = false;
        continue;
      }
      out->decisions[call] = (int)pb.negotiate(sb, rb, eligible, 0, 7, 0, 20.0, [] {}, ps, pr, &vec, form, &mine,
                                                out->rows[call]);
      out->capture[call] = varblock_any_capturing(n, out->rows[call]);
    }
    b.barrier();
  } catch (const std::exception& e) {
    fprintf(stderr, "board rank %d: %s\n", rank, e.what());
    out->threw = true;
  }
}

int check_board(int port) {
  const int n = 4;
  std::vector<BoardOut> outs((size_t)n);
  for (BoardOut& o : outs) memset((void*)&o, 0, sizeof o);
  std::vector<std::thread> th;
  for (int r = 0; r < n; ++r) th.emplace_back(board_rank, r, n, port, &outs[(size_t)r]);
  for (std::thread& t : th) t.join();
  int bad = 0;
  const int want[5] = {1, -1, 0, 0, 1};  // kRead, kMismatch, kFallback, kFallback, kRead
  for (int r = 0; r < n; ++r) {
    const BoardOut& o = outs[(size_t)r];
    bad += expect(!o.threw, "the board came up and no rendezvous threw");
    if (o.threw) continue;
    for (int call = 0; call < 5; ++call) {
      if (o.decisions[call] != want[call]) {
        fprintf(stderr, "board: rank %d call %d: decision %d, expected %d\n", r, call, o.decisions[call], want[call]);
        ++bad;
      }
      if (call == 4) continue;
      bad += expect(o.capture[call] == (call == 2), "the capture verdict is the same on every rank");
      // every rank holds the same matrix: compare with rank 0's copy and with what was published
      bad += expect(memcmp(o.rows[call], outs[0].rows[call], sizeof(mnccl::VarRow) * n) == 0, "same rows on every rank");
      for (int q = 0; q < n; ++q)
        for (int p = 0; p < n; ++p) {
          bad += expect(o.rows[call][q].sendcounts[p] == (uint64_t)(100 * call + 10 * q + p), "published sendcounts");
          bad += expect(o.rows[call][q].rdispls[p] == (uint64_t)(1000 * q + p), "published rdispls");
        }
    }
  }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  int bad = 0, cases = 0;
  for (int n : {1, 2, 3, 5, 8, 16})
    for (int kind = 0; kind < 4; ++kind)
      for (int mode = 0; mode < 3; ++mode)
        for (uint64_t slice : {(uint64_t)16, (uint64_t)1024}) {
          if (slice == 16 && n > 5 && kind == 0) continue;  // (minutes under the sanitizers)
          const uint64_t seed = (uint64_t)(1 + cases);
          bad += run_case(n, mode == 1 ? 2 : 4, kind, mode, slice, seed % 2 ? 1 : 4, {0, 2}, seed);
          bad += run_case(n, 4, kind, mode, slice, 4, {2, 2, 0}, seed + 100);
          cases += 2;
        }
  bad += check_rules();
  bad += check_board(argc > 1 ? atoi(argv[1]) : 21000 + (int)(getpid() % 20000));
  if (bad) {
    fprintf(stderr, "alltoallv selftest: %d failures (%d simulator cases)\n", bad, cases);
    return 1;
  }
  printf("alltoallv selftest: ok (%d simulator cases)\n", cases);
  return 0;
}
