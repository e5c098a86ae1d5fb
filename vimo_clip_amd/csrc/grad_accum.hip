// K20 — gradient accumulation over micro-batches on the flat gradient arena (include/vmc.h): one streaming pass that folds the
// gradient a backward has just written into an fp32 accumulator, or finishes the weighted sum in place.
//   mode 0  acc[i] = weight * g[i]                    8 B per element   (first micro-step: acc needs no zeroing)
//   mode 1  acc[i] = fmaf(weight, g[i], acc[i])      12 B per element
//   mode 2  out[i] = fmaf(weight, g[i], acc[i])      12 B per element   (last micro-step; out may be g itself)
// The multiply-add is written as fmaf, not as `weight * g + acc`: one rounding per element whatever -ffp-contract says, so the
// numbers do not depend on how this file is compiled.  Mode 0 is a single multiply, which has nothing to contract.
// Pure streaming, no reuse: 16-byte loads and stores, a grid-stride loop over a grid sized to the chip (256 CUs x 8 workgroups of
// 256 threads, the geometry of adam_kernel in train.hip) with two float4 of every stream in flight per thread to cover the HBM
// latency; the n % 4 tail is done element by element by the first workgroup.  Plain vector stores, no LDS, no atomics, and nothing
// is read from the environment.  A thread loads every element it is going to overwrite before it stores, so out == g is safe.
#include "common.h"

template <int MODE>
__device__ __forceinline__ float accum_element(float w, float g, float a) {
  return MODE == 0 ? w * g : fmaf(w, g, a);
}

template <int MODE>
__global__ void __launch_bounds__(256) grad_accum_kernel(const float* g, float* __restrict__ acc, float* out, size_t n, float w) {
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float* dst = MODE == 2 ? out : acc;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const bool two = i1 < n4;
    float4 gg[2], aa[2];
    gg[0] = ((const float4*)g)[i0];
    if (MODE != 0) aa[0] = ((const float4*)acc)[i0];
    if (two) {
      gg[1] = ((const float4*)g)[i1];
      if (MODE != 0) aa[1] = ((const float4*)acc)[i1];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float4 r;
      r.x = accum_element<MODE>(w, gg[u].x, MODE ? aa[u].x : 0.f);
      r.y = accum_element<MODE>(w, gg[u].y, MODE ? aa[u].y : 0.f);
      r.z = accum_element<MODE>(w, gg[u].z, MODE ? aa[u].z : 0.f);
      r.w = accum_element<MODE>(w, gg[u].w, MODE ? aa[u].w : 0.f);
      ((float4*)dst)[u ? i1 : i0] = r;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t k = (n4 << 2) + threadIdx.x;
    dst[k] = accum_element<MODE>(w, g[k], MODE ? acc[k] : 0.f);
  }
}

extern "C" int vmc_grad_accumulate(const float* g, float* acc, float* out, size_t n, float weight, int mode, void* stream) {
  if (!g || !acc || !out || mode < 0 || mode > 2) return VMC_E_ARG;
  if (((uintptr_t)g | (uintptr_t)acc | (uintptr_t)out) & 15) return VMC_E_ALIGN;
  if (n == 0) return 0;
  const dim3 grid(grid_for((n + 3) / 4, 512, 256 * 8)), block(256);      // 512 float4 per workgroup and trip
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case 0: hipLaunchKernelGGL(grad_accum_kernel<0>, grid, block, 0, s, g, acc, out, n, weight); break;
    case 1: hipLaunchKernelGGL(grad_accum_kernel<1>, grid, block, 0, s, g, acc, out, n, weight); break;
    default: hipLaunchKernelGGL(grad_accum_kernel<2>, grid, block, 0, s, g, acc, out, n, weight); break;
  }
  VMC_CHECK_LAUNCH();
  return 0;
}
