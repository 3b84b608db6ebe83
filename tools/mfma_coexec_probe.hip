// mfma_coexec_probe.hip -- how much MFMA time the S-box carry chains of the Poseidon kernels can hide, three cases:
//  (a) two waves of one SIMD in opposite roles: one issues the kernels' int8 MFMA stream (v_mfma_i32_16x16x64_i8 on
//      four independent accumulators, one per set), the other S-box carry chains (poseidon::sbox_n<4>, gl::mul_n);
//  (b) one wave per SIMD issuing NM MFMAs and then independent S-box chains per iteration;
//  (c) (b) with two waves per SIMD, one of them raised by s_setprio.
// Every figure is SIMD cycles per iteration of one wave (the chip's clock is read from the device attributes), the time
// of the whole launch over the iterations.  An MFMA "costs" what adding it to the VALU-only loop adds.
// Build (both: __graft_entry__.build does it):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I proof_protocol_decoder_amd/csrc -mllvm -amdgpu-mfma-vgpr-form=1
//     -o tools/mfma_coexec_probe tools/mfma_coexec_probe.hip              (accumulators in VGPRs, as the kernels)
//   the same without the -mllvm flag -o tools/mfma_coexec_probe_agpr   (accumulators in AGPRs)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include "gl.hpp"
#include "poseidon.cuh"

typedef int v4i __attribute__((ext_vector_type(4)));
constexpr int ITERS = 4096;
#ifndef MFMA_FORM
#define MFMA_FORM "VGPRs"  // the build of the AGPR form passes -DMFMA_FORM="AGPRs"
#endif

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                      \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

// NM MFMAs on four independent accumulators (the kernels' four sets), operands held in registers
template <int NM>
__device__ __forceinline__ void mfmas(v4i (&acc)[4], const v4i& a, const v4i& b) {
#pragma unroll
  for (int k = 0; k < NM; k++) acc[k & 3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[k & 3], 0, 0, 0);
}

__device__ __forceinline__ void sink(uint64_t* out, const v4i (&acc)[4], const uint64_t (&x)[4]) {
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) s += x[i] + (uint32_t)(acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3]);
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// (a) waves 0..3 (one per SIMD) run MFMAs if M, waves 4..7 (their SIMD partners) S-box chains if V
template <bool M, bool V>
__global__ void __launch_bounds__(512) roles_kernel(uint64_t* out) {
  const uint32_t t = threadIdx.x, w = t >> 6;
  uint64_t x[4] = {t + 3, t * 7 + 5, t * 11 + 1, t * 13 + 9};
  v4i acc[4] = {}, a = {(int)t, (int)t * 3, 5, 7}, b = {(int)t * 5, 1, (int)t, 9};
  if (w < 4) {
    if (M)
      for (int i = 0; i < ITERS; i++) mfmas<24>(acc, a, b);
  } else {
    if (V)
      for (int i = 0; i < ITERS; i++) poseidon::sbox_n<4>(x);
  }
  sink(out, acc, x);
}

// (b) one wave per SIMD: NM MFMAs, then S-box chains that do not depend on them (VALU = false: MFMAs only)
template <int NM, bool VALU>
__global__ void __launch_bounds__(256) mix_kernel(uint64_t* out) {
  const uint32_t t = threadIdx.x;
  uint64_t x[4] = {t + 3, t * 7 + 5, t * 11 + 1, t * 13 + 9};
  v4i acc[4] = {}, a = {(int)t, (int)t * 3, 5, 7}, b = {(int)t * 5, 1, (int)t, 9};
  for (int i = 0; i < ITERS; i++) {
    mfmas<NM>(acc, a, b);
    if (VALU) poseidon::sbox_n<4>(x);
  }
  sink(out, acc, x);
}

// (c) two waves per SIMD, both as (b) with NM = 6; waves 4..7 raise their priority to PRIO
template <int PRIO>
__global__ void __launch_bounds__(512) prio_kernel(uint64_t* out) {
  const uint32_t t = threadIdx.x;
  if (PRIO && (t >> 6) >= 4) __builtin_amdgcn_s_setprio(PRIO);
  uint64_t x[4] = {t + 3, t * 7 + 5, t * 11 + 1, t * 13 + 9};
  v4i acc[4] = {}, a = {(int)t, (int)t * 3, 5, 7}, b = {(int)t * 5, 1, (int)t, 9};
  for (int i = 0; i < ITERS; i++) {
    mfmas<6>(acc, a, b);
    poseidon::sbox_n<4>(x);
  }
  sink(out, acc, x);
}

static int n_cu = 0;
static double clock_ghz = 0;
static uint64_t* d_out = nullptr;

// SIMD cycles per iteration of one wave: the launch's time (best of 5) over ITERS
template <typename K>
static double cycles(K kernel, int threads) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  float best = 1e30f;
  for (int r = 0; r < 6; r++) {
    hipEventRecord(e0);
    hipLaunchKernelGGL(kernel, dim3(n_cu), dim3(threads), 0, 0, d_out);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    if (r && ms < best) best = ms;  // the first launch warms up
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return best * 1e-3 * clock_ghz * 1e9 / ITERS;
}

int main() {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  n_cu = p.multiProcessorCount;
  clock_ghz = p.clockRate * 1e-6;
  CHECK(hipMalloc(&d_out, (size_t)n_cu * 512 * sizeof(uint64_t)));
  printf("# %s, %d CUs, clock %.3f GHz (device attribute), one workgroup per CU, %d iterations; accumulators in %s\n",
         p.gcnArchName, n_cu, clock_ghz, ITERS, MFMA_FORM);
  printf("(a) opposite roles on one SIMD (24 MFMAs vs one sbox_n<4> per iteration)\n");
  const double a_m = cycles(roles_kernel<true, false>, 512), a_v = cycles(roles_kernel<false, true>, 512),
               a_mv = cycles(roles_kernel<true, true>, 512);
  printf("    MFMA wave alone %8.1f  VALU wave alone %8.1f  both %8.1f  -> hidden %.0f %% of the shorter\n", a_m, a_v,
         a_mv, 100.0 * (a_m + a_v - a_mv) / (a_m < a_v ? a_m : a_v));
  printf("(b) one wave per SIMD: NM MFMAs + one sbox_n<4> per iteration\n");
  const double v0 = cycles(mix_kernel<0, true>, 256);
  const double m6 = cycles(mix_kernel<6, false>, 256), b6 = cycles(mix_kernel<6, true>, 256);
  const double m24 = cycles(mix_kernel<24, false>, 256), b24 = cycles(mix_kernel<24, true>, 256);
  printf("    VALU only %8.1f\n", v0);
  printf("    NM =  6: MFMA only %8.1f  mixed %8.1f  -> %.1f cycles per MFMA beside VALU\n", m6, b6, (b6 - v0) / 6);
  printf("    NM = 24: MFMA only %8.1f  mixed %8.1f  -> %.1f cycles per MFMA beside VALU\n", m24, b24, (b24 - v0) / 24);
  printf("(c) two waves per SIMD, each NM = 6 + one sbox_n<4>; waves 4..7 at s_setprio PRIO\n");
  const double c0 = cycles(prio_kernel<0>, 512), c3 = cycles(prio_kernel<3>, 512);
  printf("    PRIO 0 %8.1f  PRIO 3 %8.1f  (cycles per iteration of the slower wave pair; 2 x (b) NM = 6 = %.1f)\n", c0,
         c3, 2 * b6);
  CHECK(hipFree(d_out));
  return 0;
}
