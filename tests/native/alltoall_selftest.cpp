// alltoall_selftest.cpp -- the simulator's all-to-all (csrc/sim.cpp mnccl_sim_mixed: schedule.h's
// hop table on the ring, the mirror of kernels.hip exchange_push on the read schedule) run under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_alltoall_cpu.py.  A stand-alone
// program: a handful of the CPU suite's simulator cases, random bytes in, the permutation out,
// guard bytes behind every recv.  Exits non-zero on any mismatch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" int mnccl_sim_mixed(int n, int calls, const int* coll, const int* sched, const uint64_t* counts,
                               const int* roots, const float* const* send, float* const* recv, int op,
                               uint64_t slice_bytes, uint64_t min_slice, int channels, int slots, uint64_t schedule_seed,
                               uint64_t* steps_out);

namespace {

constexpr size_t kGuard = 256;
constexpr unsigned char kGuardByte = 0xA5;

uint64_t next(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// `calls` calls on one communicator state: all-to-alls of `count` fp32 words per block on the given
// schedules, an all-gather of the same count between them when `with_gather`
int run_case(int n, uint64_t count, uint64_t slice, int channels, int slots, const std::vector<int>& scheds,
             bool with_gather, uint64_t seed) {
  const size_t block = (size_t)count * 4, bytes = block * (size_t)n;
  std::vector<int> coll, sched, roots;
  std::vector<uint64_t> counts;
  for (size_t i = 0; i < scheds.size(); ++i) {
    coll.push_back(with_gather && i == 1 ? 2 : 5);
    sched.push_back(scheds[i]);
    roots.push_back(0);
    counts.push_back(count);
  }
  const size_t k = coll.size();
  // float storage keeps the buffers 4-byte aligned, as the simulator's word copies need
  std::vector<std::vector<float>> send(k * n), recv(k * n);
  std::vector<const float*> sp(k * n);
  std::vector<float*> rp(k * n);
  uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 1;
  for (size_t i = 0; i < k; ++i)
    for (int r = 0; r < n; ++r) {
      const size_t sb = coll[i] == 5 ? bytes : block;  // an all-gather's send holds one block
      std::vector<float>& s = send[i * n + r];
      std::vector<float>& d = recv[i * n + r];
      s.resize(sb / 4);
      for (size_t b = 0; b < sb; ++b) ((unsigned char*)s.data())[b] = (unsigned char)next(rng);
      d.resize((bytes + kGuard) / 4);
      memset(d.data(), kGuardByte, bytes + kGuard);
      sp[i * n + r] = s.data();
      rp[i * n + r] = d.data();
    }
  std::vector<std::vector<float>> before = send;
  uint64_t steps = 0;
  const int rc = mnccl_sim_mixed(n, (int)k, coll.data(), sched.data(), counts.data(), roots.data(), sp.data(), rp.data(),
                                 0, slice, 0, channels, slots, seed, &steps);
  if (rc != 0) {
    fprintf(stderr, "n=%d count=%llu slice=%llu: rc %d\n", n, (unsigned long long)count, (unsigned long long)slice, rc);
    return 1;
  }
  for (size_t i = 0; i < k; ++i)
    for (int q = 0; q < n; ++q) {
      const unsigned char* d = (const unsigned char*)recv[i * n + q].data();
      for (int r = 0; r < n; ++r) {
        // block r of rank q's recv: block q of rank r's send (all-gather: rank r's one block)
        const unsigned char* s = (const unsigned char*)send[i * n + r].data() + (coll[i] == 5 ? (size_t)q * block : 0);
        if (memcmp(d + (size_t)r * block, s, block) != 0) {
          fprintf(stderr, "n=%d count=%llu call %zu: block %d of rank %d's recv differs\n", n,
                  (unsigned long long)count, i, r, q);
          return 1;
        }
      }
      for (size_t g = 0; g < kGuard; ++g)
        if (d[bytes + g] != kGuardByte) {
          fprintf(stderr, "n=%d call %zu: rank %d's guard bytes were written\n", n, i, q);
          return 1;
        }
      if (memcmp(send[i * n + q].data(), before[i * n + q].data(), send[i * n + q].size() * 4) != 0) {
        fprintf(stderr, "n=%d call %zu: rank %d's send was written\n", n, i, q);
        return 1;
      }
    }
  return 0;
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  const int ns[] = {1, 2, 3, 5, 8, 16};
  const uint64_t counts[] = {1, 3, 300, 16411};
  for (int n : ns)
    for (uint64_t count : counts)
      for (uint64_t slice : {(uint64_t)16, (uint64_t)1024}) {
        if (count == 16411 && slice == 16 && n > 5) continue;  // (minutes under the sanitizers)
        for (uint64_t seed = 1; seed <= 2; ++seed) {
          const int channels = seed == 1 ? 1 : 4;
          bad += run_case(n, count, slice, channels, 2, {0, 2}, false, seed);
          bad += run_case(n, count, slice, channels, 1, {2, 2}, false, seed);  // read needs no slots
          cases += 2;
        }
      }
  // sequences on one state: ring, all-gather, read, ring
  for (int n : {2, 4, 9}) {
    bad += run_case(n, 700, 128, 4, 2, {0, 2, 2, 0}, true, 7);
    bad += run_case(n, 700, 128, 3, 2, {2, 0, 0, 2}, true, 8);
    cases += 2;
  }
  if (bad) {
    fprintf(stderr, "alltoall selftest: %d of %d cases failed\n", bad, cases);
    return 1;
  }
  printf("alltoall selftest: ok (%d cases)\n", cases);
  return 0;
}
