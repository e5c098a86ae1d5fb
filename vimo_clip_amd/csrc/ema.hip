// K22 — exponential moving average of the fp32 masters on the flat parameter arena (include/vmc.h), and the exchange of two fp32
// buffers that lets an evaluation run on the average without a third arena-sized buffer.
//   vmc_ema_update   ema[i] = fmaf(w, p[i] - ema[i], ema[i])      12 B per element   (torch.lerp(ema, p, w))
//   vmc_ema_swap     a[i] <-> b[i], bit for bit                   16 B per element
// The update is one subtraction and one explicit fmaf: two roundings per element whatever -ffp-contract says (there is no separate
// multiply to contract), so the numbers do not depend on how this file is compiled.  w is 1 - decay as the HOST rounded it from
// float64 (an fp32 `1 - 0.9999f` is off by 6e-4 relative), or with warm-up max(1 - decay, 9 / (10 + t)): decay_t = min(decay,
// (1 + t) / (10 + t)) written without the cancellation.  t comes from the argument or, for captured steps, from state[0] of
// vmc_train_tick in device memory; every thread computes the same w from the same words.  A skip flag in device memory (the
// found_inf word of vmc_loss_scale_state) makes every workgroup return before its first store: the contract of
// vmc_adam_step_dev_skip.
// Both kernels have the shape of grad_accum_kernel: pure streaming, 16-byte loads and stores, a grid-stride loop over a grid sized to
// the chip (256 CUs x 8 workgroups of 256 threads) with two float4 of every stream in flight per thread, the n % 4 tail element by
// element by the first workgroup.  Plain vector stores, no LDS, no atomics, nothing read from the environment.  A thread loads
// every element it is going to overwrite before it stores.
#include "common.h"

__device__ __forceinline__ float ema_element(float w, float p, float e) { return fmaf(w, p - e, e); }

__global__ void __launch_bounds__(256) ema_update_kernel(float* ema, const float* p, size_t n, float one_minus_decay, int warmup,
                                                         long long step, const long long* state, const int* skip) {
  if (skip != nullptr && *skip != 0) return;      // a skipped step: uniform, before any store
  float w = one_minus_decay;
  if (warmup) {
    const long long t = state != nullptr ? *state : step;
    w = fmaxf(one_minus_decay, 9.0f / (float)(10 + t));
  }
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const bool two = i1 < n4;
    float4 pp[2], ee[2];
    pp[0] = ((const float4*)p)[i0];
    ee[0] = ((const float4*)ema)[i0];
    if (two) {
      pp[1] = ((const float4*)p)[i1];
      ee[1] = ((const float4*)ema)[i1];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float4 r;
      r.x = ema_element(w, pp[u].x, ee[u].x);
      r.y = ema_element(w, pp[u].y, ee[u].y);
      r.z = ema_element(w, pp[u].z, ee[u].z);
      r.w = ema_element(w, pp[u].w, ee[u].w);
      ((float4*)ema)[u ? i1 : i0] = r;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t k = (n4 << 2) + threadIdx.x;
    ema[k] = ema_element(w, p[k], ema[k]);
  }
}

// Bits, not values: the words travel as 32-bit integers, so NaN payloads, -0 and subnormals arrive as they left.
__global__ void __launch_bounds__(256) ema_swap_kernel(unsigned* a, unsigned* b, size_t n) {
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const bool two = i1 < n4;
    const uint4 a0 = ((const uint4*)a)[i0];
    const uint4 b0 = ((const uint4*)b)[i0];
    uint4 a1 = a0, b1 = b0;                        // named registers, not arrays: an indexed array may be promoted to LDS
    if (two) {
      a1 = ((const uint4*)a)[i1];
      b1 = ((const uint4*)b)[i1];
    }
    ((uint4*)a)[i0] = b0;
    ((uint4*)b)[i0] = a0;
    if (two) {
      ((uint4*)a)[i1] = b1;
      ((uint4*)b)[i1] = a1;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t k = (n4 << 2) + threadIdx.x;
    const unsigned x = a[k], y = b[k];
    a[k] = y;
    b[k] = x;
  }
}

extern "C" int vmc_ema_update(float* ema, const float* p, size_t n, float one_minus_decay, int warmup, long long step,
                              const void* train_state, const int* skip, void* stream) {
  if (!ema || !p || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f) || (warmup != 0 && warmup != 1) || step < 0) return VMC_E_ARG;
  if ((((uintptr_t)ema | (uintptr_t)p) & 15) || ((uintptr_t)train_state & 7) || ((uintptr_t)skip & 3)) return VMC_E_ALIGN;
  if (n == 0) return 0;
  const dim3 grid(grid_for((n + 3) / 4, 512, 256 * 8)), block(256);      // 512 float4 per workgroup and trip
  hipLaunchKernelGGL(ema_update_kernel, grid, block, 0, (hipStream_t)stream, ema, p, n, one_minus_decay, warmup, step,
                     (const long long*)train_state, skip);
  VMC_CHECK_LAUNCH();
  return 0;
}

extern "C" int vmc_ema_swap(float* a, float* b, size_t n, void* stream) {
  if (!a || !b || a == b) return VMC_E_ARG;
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  if (ua < ub + bytes && ub < ua + bytes) return VMC_E_ARG;             // the ranges overlap
  if ((ua | ub) & 15) return VMC_E_ALIGN;
  if (n == 0) return 0;
  const dim3 grid(grid_for((n + 3) / 4, 512, 256 * 8)), block(256);
  hipLaunchKernelGGL(ema_swap_kernel, grid, block, 0, (hipStream_t)stream, (unsigned*)a, (unsigned*)b, n);
  VMC_CHECK_LAUNCH();
  return 0;
}
