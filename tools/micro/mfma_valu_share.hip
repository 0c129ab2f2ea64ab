// mfma_valu_share.hip — do fp64 vector and fp64 matrix instructions share issue on a gfx950 SIMD?  (kernels_as.hip: the factor sweep is
// bound by its vector port at 4 waves per SIMD — would moving data with MFMA "selector" products instead of vector moves be free?)
// One workgroup of 1024 threads per CU: 16 waves, 4 per SIMD (wave w of a workgroup lands on SIMD w % 4; the tool reads the hardware
// id of every wave and checks it).  Waves 0-3 and 8-11 have role V, waves 4-7 and 12-15 role M: every SIMD holds two of each.
// Loops of EQUAL trip count, all operands in registers, independent accumulator chains:
//   V only   role V runs v_fma_f64 (8 chains, 64 per trip), role M leaves at once
//   M only   role M runs v_mfma_f64_16x16x4_f64 (4 chains, 4 per trip), role V leaves at once
//   V + M    both roles run, from different waves of the same SIMD
//   V x 4, M x 4   all four waves of a SIMD in one role (does a role saturate with two waves?)
// t(V + M) ~ t(V) + t(M): the two share issue; an MFMA then costs t(M) / t(V) * (64 / 4) vector instructions of this kind.
// t(V + M) ~ max: they overlap, matrix work next to a busy vector port is free.
//   hipcc -O3 --offload-arch=gfx950 tools/micro/mfma_valu_share.hip -o tools/micro/mfma_valu_share
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int CV = 8, NV = 64, NM = 4;  // chains of role V; instructions per trip of role V / M (by the data sheet an MFMA takes 16 v_fma_f64: equal times)
#define OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(hipGetLastError())); return 1; } } while (0)

// mode bit 0: role V works, bit 1: role M works, bit 2: every wave takes the role named by bits 0 / 1
__global__ void __launch_bounds__(1024) k_share(int mode, int trips, double seed, double *sink, unsigned *where) {
  const int wave = threadIdx.x >> 6;
  const bool role_m = (mode & 4) ? (mode & 2) != 0 : ((wave >> 2) & 1) != 0;
  if ((threadIdx.x & 63) == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    where[blockIdx.x * 16 + wave] = ((xcc & 0xF) << 16) | (hw & 0xFF30) | (role_m ? 1u : 0u);  // xcc | se sh cu . simd | role
  }
  if (!(mode & 4) && !(mode & (role_m ? 2 : 1))) return;
  const double x = seed + 1e-9 * threadIdx.x, y = 1.0 - 1e-7 * (threadIdx.x & 15);
  double r = 0.0;
  if (!role_m) {
    double a[CV];
#pragma unroll
    for (int k = 0; k < CV; k++) a[k] = x + k;
    for (int t = 0; t < trips; t++) {
#pragma unroll
      for (int k = 0; k < NV; k++) a[k % CV] = __builtin_fma(a[k % CV], y, x);
    }
#pragma unroll
    for (int k = 0; k < CV; k++) r += a[k];
  } else {
    v4d c[NM];
#pragma unroll
    for (int k = 0; k < NM; k++) c[k] = (v4d){x, x + k, 0.0, 1.0};
    for (int t = 0; t < trips; t++) {
#pragma unroll
      for (int k = 0; k < NM; k++) c[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(y, x, c[k], 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < NM; k++) r += c[k][0] + c[k][1] + c[k][2] + c[k][3];
  }
  if (r == 12345.678) sink[0] = r;  // (never: keeps the chains alive)
}

int main(int argc, char **argv) {
  const int trips = argc > 1 ? atoi(argv[1]) : 5000, reps = 5;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
  const int B = prop.multiProcessorCount;
  double *sink;
  unsigned *where;
  if (hipMalloc(&sink, 8) != hipSuccess || hipMalloc(&where, (size_t)B * 16 * sizeof(unsigned)) != hipSuccess) return 1;
  hipEvent_t e0, e1;
  OK(hipEventCreate(&e0)); OK(hipEventCreate(&e1));
  struct Case { const char *name; int mode; } cases[] = {{"V only (2 waves per SIMD)", 1}, {"M only (2 waves per SIMD)", 2}, {"V + M  (2 + 2 waves per SIMD)", 3},
                                                         {"V x 4  (4 waves per SIMD)", 4 | 1}, {"M x 4  (4 waves per SIMD)", 4 | 2}};
  double best[5];
  printf("%s: %d CUs, one 1024-thread workgroup each, %d trips of %d v_fma_f64 / %d v_mfma_f64_16x16x4_f64, best of %d launches\n", prop.name, B, trips, NV, NM, reps);
  for (int k = 0; k < 5; k++) {
    best[k] = 1e30;
    for (int r = 0; r < reps + 1; r++) {  // (first launch: warm-up)
      OK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(k_share, dim3(B), dim3(1024), 0, 0, cases[k].mode, trips, 0.5, sink, where);
      OK(hipEventRecord(e1, 0));
      OK(hipEventSynchronize(e1));
      float ms = 0.f;
      OK(hipEventElapsedTime(&ms, e0, e1));
      if (r > 0) best[k] = std::min(best[k], (double)ms);
    }
    printf("  %-32s %8.3f ms\n", cases[k].name, best[k]);
  }
  // placement of the last mixed launch's waves: per SIMD, how many waves of each role
  hipLaunchKernelGGL(k_share, dim3(B), dim3(1024), 0, 0, 3, 1, 0.5, sink, where);
  OK(hipDeviceSynchronize());
  std::vector<unsigned> h((size_t)B * 16);
  OK(hipMemcpy(h.data(), where, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
  std::map<unsigned, std::pair<int, int>> simd;
  for (unsigned v : h) { auto &p = simd[v & ~1u]; (v & 1 ? p.second : p.first)++; }
  int even = 0;
  for (auto &kv : simd) even += kv.second.first == 2 && kv.second.second == 2;
  printf("placement: %zu SIMDs hold waves, %d of them exactly 2 V + 2 M\n", simd.size(), even);
  const double tv = best[0], tm = best[1], tb = best[2];
  printf("t(V + M) / (t(V) + t(M)) = %.3f    t(V + M) / max(t(V), t(M)) = %.3f\n", tb / (tv + tm), tb / std::max(tv, tm));
  printf("per instruction and SIMD, two waves: v_fma_f64 %.2f ns, MFMA %.2f ns -> one MFMA takes the time of %.1f v_fma_f64\n", 1e6 * tv / ((double)trips * NV * 2),
         1e6 * tm / ((double)trips * NM * 2), (tm / NM) / (tv / NV));
  printf("four waves in one role: V x 4 / V only = %.2f, M x 4 / M only = %.2f (2.00: two waves already fill the unit)\n", best[3] / tv, best[4] / tm);
  OK(hipFree(sink)); OK(hipFree(where));
  return 0;
}
