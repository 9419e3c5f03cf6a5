// split_selftest.cpp -- ncclCommSplit's host side under AddressSanitizer +
// UndefinedBehaviorSanitizer, run by tests/test_split_cpu.py.  A stand-alone program (its own main;
// csrc/bootstrap.cpp is the only other source, no HIP):
//  * the plan (csrc/split.h split_plan) for n = 1 ... 16 over seeded random colors and keys, plus
//    all-equal keys, negative keys, every rank NCCL_SPLIT_NOCOLOR and every rank its own color,
//    against a sort-based restatement: the groups partition the coloured ranks, the new ranks are
//    0 ... size - 1 in (key, parent rank) order, the leader is new rank 0;
//  * the two-round bootstrap (csrc/bootstrap.h split_bootstrap), 5 ranks as threads over
//    127.0.0.1 with colors 0, 1, 0, -1, 1: every child star all-gathers and barriers, the parent
//    star still works afterwards, and a second split on it works too;
//  * a failure path: a leader whose members never connect -- and one whose members connect only in
//    part -- hits a short timeout, throws, and leaves no descriptor open.
// Exits non-zero on any failure.  argv[1]: the TCP port of the parent's bootstrap (default: from the pid).
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <stdexcept>
#include <thread>
#include <utility>
#include <vector>

#include "bootstrap.h"
#include "split.h"

namespace {

using mnccl::Bootstrap;
using mnccl::SplitSlot;

int fails = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++fails;                                                        \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

uint64_t next(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// the rule restated: the members of r's color, sorted by (key, parent rank)
void check_plan(const std::vector<int32_t>& colors, const std::vector<int32_t>& keys) {
  const int n = (int)colors.size();
  std::vector<SplitSlot> plan((size_t)n);
  mnccl::split_plan(n, colors.data(), keys.data(), plan.data());
  for (int r = 0; r < n; ++r) {
    const SplitSlot s = plan[(size_t)r];
    if (colors[(size_t)r] < 0) {
      CHECK(s.size == 0 && s.rank == -1 && s.leader == -1);
      continue;
    }
    std::vector<std::pair<int32_t, int>> members;
    for (int q = 0; q < n; ++q)
      if (colors[(size_t)q] == colors[(size_t)r]) members.emplace_back(keys[(size_t)q], q);
    std::sort(members.begin(), members.end());
    CHECK(s.size == (int)members.size());
    CHECK(s.rank >= 0 && s.rank < s.size && members[(size_t)s.rank].second == r);
    CHECK(s.leader == members[0].second);
    CHECK(plan[(size_t)s.leader].rank == 0 && colors[(size_t)s.leader] == colors[(size_t)r]);
  }
}

void plan_cases() {
  uint64_t rng = 12345;
  for (int n = 1; n <= 16; ++n) {
    std::vector<int32_t> colors((size_t)n), keys((size_t)n);
    for (int round = 0; round < 20; ++round) {
      const int ncolors = 1 + (int)(next(rng) % (uint64_t)n);
      for (int r = 0; r < n; ++r) {
        // one rank in five joins no group; keys in [-3, 3]: negative ones and many ties
        colors[(size_t)r] = next(rng) % 5 == 0 ? mnccl::kSplitNoColor : (int32_t)(next(rng) % (uint64_t)ncolors) * 7;
        keys[(size_t)r] = (int32_t)(next(rng) % 7) - 3;
      }
      check_plan(colors, keys);
    }
    for (int r = 0; r < n; ++r) colors[(size_t)r] = r % 2, keys[(size_t)r] = 5;  // all-equal keys
    check_plan(colors, keys);
    for (int r = 0; r < n; ++r) keys[(size_t)r] = -r;  // negative keys: every group reversed
    check_plan(colors, keys);
    for (int r = 0; r < n; ++r) keys[(size_t)r] = r % 3 == 0 ? INT32_MIN : INT32_MAX;  // the extremes
    check_plan(colors, keys);
    for (int r = 0; r < n; ++r) colors[(size_t)r] = mnccl::kSplitNoColor;  // nobody joins
    check_plan(colors, keys);
    for (int r = 0; r < n; ++r) colors[(size_t)r] = n - r;  // every rank its own color
    check_plan(colors, keys);
  }
}

int open_fds() {
  int k = 0;
  DIR* d = opendir("/proc/self/fd");
  if (!d) return -1;
  while (readdir(d)) ++k;
  closedir(d);
  return k;  // (".", ".." and the directory's own descriptor: the same every time)
}

// one rank's split and its child star's all-gather (parent ranks, in the plan's order) and barrier
int split_round(Bootstrap& parent, const std::vector<int32_t>& colors, const std::vector<int32_t>& keys) {
  const int n = parent.nranks(), me = parent.rank();
  std::vector<SplitSlot> plan((size_t)n);
  mnccl::split_plan(n, colors.data(), keys.data(), plan.data());
  Bootstrap child;
  int port = -1;
  const SplitSlot s = mnccl::split_bootstrap(parent, colors[(size_t)me], keys[(size_t)me], 20.0, &child, &port);
  const SplitSlot want = plan[(size_t)me];
  if (s.size != want.size || s.rank != want.rank || s.leader != want.leader) return 2;
  if (s.size == 0) return child.nranks() == 0 && port == 0 ? 0 : 4;
  if (child.rank() != s.rank || child.nranks() != s.size || (s.size == 1) != (port == 0)) return 4;
  const int32_t mine = me;
  std::vector<int32_t> all((size_t)s.size, -1);
  child.allgather(&mine, all.data(), sizeof mine);
  child.barrier();
  for (int q = 0; q < n; ++q)
    if (plan[(size_t)q].size > 0 && plan[(size_t)q].leader == s.leader && all[(size_t)plan[(size_t)q].rank] != q) return 3;
  return 0;
}

void two_rounds(int port) {
  const std::vector<int32_t> colors = {0, 1, 0, mnccl::kSplitNoColor, 1}, keys = {2, -1, 2, 9, -4};
  const std::vector<int32_t> own = {4, 3, 2, 1, 0};  // the second split: every rank its own color
  const int n = (int)colors.size();
  std::vector<int> rcs((size_t)n, -1);
  auto rank_main = [&](int r) {
    try {
      Bootstrap parent;
      parent.connect(r, n, "127.0.0.1", port, 20.0);
      int rc = split_round(parent, colors, keys);
      const int32_t mine = 100 + r;
      std::vector<int32_t> all((size_t)n, -1);
      parent.allgather(&mine, all.data(), sizeof mine);  // the parent star still works
      for (int q = 0; q < n && rc == 0; ++q)
        if (all[(size_t)q] != 100 + q) rc = 5;
      if (rc == 0) rc = split_round(parent, own, keys);   // singletons: no socket at all
      if (rc == 0) rc = split_round(parent, colors, own);  // and groups again, other keys
      parent.barrier();
      rcs[(size_t)r] = rc;
    } catch (const std::exception& e) {
      fprintf(stderr, "rank %d: %s\n", r, e.what());
      rcs[(size_t)r] = 1;
    }
  };
  std::vector<std::thread> ts;
  for (int r = 0; r < n; ++r) ts.emplace_back(rank_main, r);
  for (auto& t : ts) t.join();
  for (int r = 0; r < n; ++r) CHECK(rcs[(size_t)r] == 0);
}

void leader_timeouts() {
  const int before = open_fds();
  CHECK(before > 0);
  {
    // nobody connects
    Bootstrap lead;
    const int port = lead.listen_on(0, true);
    CHECK(port > 0);
    CHECK(open_fds() == before + 1);
    bool threw = false;
    try {
      lead.accept_members(3, 0.2);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
    CHECK(open_fds() == before);  // the listening socket went with the failure, not with the object
  }
  {
    // one of two members connects: the leader gives up on the other, and the member that did
    // connect sees its star closed instead of waiting
    Bootstrap lead, member;
    const int port = lead.listen_on(0, true);
    member.connect(1, 3, "127.0.0.1", port, 5.0);
    bool threw = false;
    try {
      lead.accept_members(3, 0.3);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
    bool member_failed = false;
    try {
      int32_t v = 1, all[3];
      member.allgather(&v, all, sizeof v);
    } catch (const std::exception&) {
      member_failed = true;
    }
    CHECK(member_failed);
    member.close_all();
    CHECK(open_fds() == before);
  }
  {
    // a moved-from star owns nothing; the moved-to one closes everything
    Bootstrap a;
    CHECK(a.listen_on(0, true) > 0);
    Bootstrap b(std::move(a));
    CHECK(open_fds() == before + 1);
    b.close_all();
    CHECK(open_fds() == before);
  }
  CHECK(open_fds() == before);
}

}  // namespace

int main(int argc, char** argv) {
  const int port = argc > 1 ? atoi(argv[1]) : 20000 + (int)(getpid() % 20000);
  plan_cases();
  const int before = open_fds();
  two_rounds(port);
  CHECK(open_fds() == before);
  leader_timeouts();
  if (fails) {
    fprintf(stderr, "split selftest: %d check(s) failed\n", fails);
    return 1;
  }
  printf("split selftest: ok\n");
  return 0;
}
