// f64 MFMA rate on gfx950: a bare loop of v_mfma_f64_16x16x4_f64 on 16 independent
// accumulator tiles per wave (the shape of k_xc_sums' inner loop, operands in registers),
// one and two waves per SIMD on every CU.  Prints one JSON line: TFLOP/s (2 x 16 x 16 x 4
// flop per wave instruction) and cycles per MFMA per SIMD at the reported clock; the f64
// matrix floor of profiles/xs_corr_time.py.  Build: hipcc --offload-arch=gfx950 -O3
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int ITER = 2048, NACC = 16;

__global__ __launch_bounds__(256) void k_mfma_f64(double* out, double a0, double b0) {
  v4d acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
  const double a = a0 + threadIdx.x, b = b0 - threadIdx.x;
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

#define CK(x)                                                              \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) {                                                \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main() {
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  const double clk = p.clockRate * 1e3;  // Hz
  double* out;
  CK(hipMalloc(&out, (size_t)cus * 2 * 256 * sizeof(double)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("{\"device\": \"%s\", \"cus\": %d, \"clock_GHz\": %.3f", p.name, cus, clk / 1e9);
  for (int wps = 1; wps <= 2; ++wps) {  // 256-thread workgroups per CU = waves per SIMD
    const int blocks = cus * wps;
    std::vector<float> ms;
    for (int r = 0; r < 7; ++r) {  // the first two are warm-up
      CK(hipEventRecord(e0));
      hipLaunchKernelGGL(k_mfma_f64, dim3(blocks), dim3(256), 0, 0, out, 1.0, 2.0);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float t;
      CK(hipEventElapsedTime(&t, e0, e1));
      if (r >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double sec = ms[ms.size() / 2] * 1e-3;
    const double per_simd = (double)wps * ITER * NACC;  // wave instructions per SIMD
    const double flops = (double)blocks * 4 * ITER * NACC * 2.0 * 16 * 16 * 4;
    printf(", \"waves_per_simd_%d\": {\"ms\": %.3f, \"TFLOPs\": %.2f, \"cycles_per_mfma\": %.1f}", wps, sec * 1e3,
           flops / sec / 1e12, sec * clk / per_simd);
  }
  printf("}\n");
  CK(hipFree(out));
  return 0;
}
