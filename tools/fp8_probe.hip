// fp8 on gfx950, two measurements (not product code):
//
//  cvt    what v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 do WITHOUT the library's clamp on overflow, inf, NaN
//         and subnormal inputs -- the record behind DESIGN.md "fp8" (the library itself never hands the
//         instruction a finite value beyond the largest finite one: kernels.hip fp8_sat).
//  bw     mncclLocalReduce bandwidth, ncclFloat8e4m3 Sum against ncclFloat16 Sum on the same bytes
//         (1 GiB per buffer by default), interleaved rounds in one process, hipEvents.
//
// Build (from the repository root, after the library):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude tools/fp8_probe.hip -o tools/bin/fp8_probe \
//         -Lmini-nccl_amd/lib -lmini_nccl -Wl,-rpath,'$ORIGIN/../../mini-nccl_amd/lib'
// Run:  tools/bin/fp8_probe cvt | tools/bin/fp8_probe bw [MiB] [rounds]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mini_nccl_api.h"
#include "mini_nccl_ext.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); return 1; } } while (0)

__global__ void cvt_kernel(const float* in, unsigned char* e4, unsigned char* e5, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e4[i] = (unsigned char)__builtin_amdgcn_cvt_pk_fp8_f32(in[i], in[i], 0, false);
  e5[i] = (unsigned char)__builtin_amdgcn_cvt_pk_bf8_f32(in[i], in[i], 0, false);
}

static int probe_cvt() {
  struct { const char* what; float v; } rows[] = {
      {"e4m3 largest finite 448", 448.f}, {"just below the e4m3 overflow midpoint", 463.99f}, {"e4m3 overflow midpoint 464", 464.f},
      {"465", 465.f}, {"480 (e4m3's NaN slot as a value)", 480.f}, {"1e4", 1e4f}, {"-1e4", -1e4f},
      {"e5m2 largest finite 57344", 57344.f}, {"61439", 61439.f}, {"e5m2 overflow midpoint 61440", 61440.f}, {"61441", 61441.f},
      {"65536", 65536.f}, {"1e9", 1e9f}, {"-1e9", -1e9f}, {"FLT_MAX", 3.4028235e38f},
      {"+inf", INFINITY}, {"-inf", -INFINITY}, {"NaN", NAN}, {"-NaN", -NAN},
      {"+0", 0.f}, {"-0", -0.f},
      {"e4m3 smallest subnormal 2^-9", 0x1p-9f}, {"tie 2^-10 (to even: 0)", 0x1p-10f}, {"tie 1.5 * 2^-9 (to even: 2)", 0x1.8p-9f},
      {"just above 2^-10", 0x1.000002p-10f}, {"-2^-11 (to -0)", -0x1p-11f},
      {"e5m2 smallest subnormal 2^-16", 0x1p-16f}, {"tie 2^-17 (to even: 0)", 0x1p-17f}, {"tie 1.5 * 2^-16", 0x1.8p-16f},
      {"f32 subnormal 2^-140", 0x1p-140f}, {"-2^-140", -0x1p-140f},
  };
  const int n = (int)(sizeof rows / sizeof rows[0]);
  std::vector<float> h(n);
  for (int i = 0; i < n; ++i) h[i] = rows[i].v;
  float* d;
  unsigned char *d4, *d5;
  CK(hipMalloc(&d, n * sizeof(float)));
  CK(hipMalloc(&d4, n));
  CK(hipMalloc(&d5, n));
  CK(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(cvt_kernel, dim3(1), dim3(64), 0, 0, d, d4, d5, n);
  CK(hipDeviceSynchronize());
  std::vector<unsigned char> r4(n), r5(n);
  CK(hipMemcpy(r4.data(), d4, n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(r5.data(), d5, n, hipMemcpyDeviceToHost));
  printf("%-44s %-14s %-8s %-8s\n", "input (no clamp ahead of the instruction)", "f32", "fp8", "bf8");
  for (int i = 0; i < n; ++i) printf("%-44s %-14.8g 0x%02x     0x%02x\n", rows[i].what, rows[i].v, r4[i], r5[i]);
  return 0;
}

static int probe_bw(size_t mib, int rounds) {
  const size_t bytes = mib << 20;
  char *a, *b;
  CK(hipMalloc(&a, bytes));
  CK(hipMalloc(&b, bytes));
  // 0x38 / 0x3c: 1.0 in e4m3 and in e5m2, a small normal f16 as two bytes: no NaN, nothing saturates early
  CK(hipMemset(a, 0x38, bytes));
  CK(hipMemset(b, 0x28, bytes));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  struct { const char* name; ncclDataType_t dt; size_t esz; } forms[] = {{"e4m3 sum", ncclFloat8e4m3, 1}, {"f16 sum", ncclFloat16, 2},
                                                                        {"e5m2 sum", ncclFloat8e5m2, 1}, {"f32 sum", ncclFloat, 4}};
  std::vector<float> ms[4];
  for (int r = 0; r < rounds + 1; ++r)
    for (int f = 0; f < 4; ++f) {
      CK(hipEventRecord(e0, st));
      if (mncclLocalReduce(a, a, b, bytes / forms[f].esz, forms[f].dt, ncclSum, st) != ncclSuccess) {
        printf("mncclLocalReduce failed for %s\n", forms[f].name);
        return 1;
      }
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      float t;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r) ms[f].push_back(t);  // (round 0 warms up: code object load, first touch)
    }
  printf("a <- a + b in place, %zu MiB per buffer, %d interleaved rounds; GB/s = 3 x bytes / time (2 reads, 1 write)\n", mib, rounds);
  for (int f = 0; f < 4; ++f) {
    std::sort(ms[f].begin(), ms[f].end());
    const double med = ms[f][ms[f].size() / 2], best = ms[f].front(), worst = ms[f].back();
    printf("%-9s median %.3f ms (%.0f GB/s)  min %.3f ms (%.0f GB/s)  max %.3f ms\n", forms[f].name, med, 3.0 * bytes / med / 1e6,
           best, 3.0 * bytes / best / 1e6, worst);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "cvt")) return probe_cvt();
  if (argc >= 2 && !strcmp(argv[1], "bw")) return probe_bw(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1024, argc > 3 ? atoi(argv[3]) : 10);
  printf("usage: %s cvt | bw [MiB] [rounds]\n", argv[0]);
  return 2;
}
