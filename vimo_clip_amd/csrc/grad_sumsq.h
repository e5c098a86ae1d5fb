// Sum of squares of the flat gradient arena, shared by vmc_grad_clip_dev (train.hip) and vmc_loss_scale_check (loss_scale.hip): one
// body, so that the two give the same bits for the same gradient -- what makes a clipped step under a power-of-two loss scale equal
// the clipped step without one (DESIGN.md "Dynamic loss scaling").
// Store and sum: every workgroup of pass one leaves the sum of squares of its grid-stride share in part[blockIdx.x]; pass two (one
// workgroup) adds the partials in a fixed order.  No atomics: the result does not depend on the order in which workgroups finish,
// so a replayed step repeats bit for bit.  A thread squares and adds in fp32 (at most a few dozen terms per accumulator even for a
// 33 M-element arena); everything that is summed across threads is a double.
#pragma once
#include "common.h"

#define CLIP_BLOCKS 2048      // 256 CUs x 8 workgroups of 256 threads

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double block_sum_f64(double a, double* sm) {      // 256 threads, sm = 4 doubles of LDS, one call per kernel
  a = wave_sum_f64(a);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// ±inf or NaN: all exponent bits set.  Tested per ELEMENT: a finite value whose fp32 square overflows is not an overflow.
__device__ __forceinline__ unsigned nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// This thread's share of sum(g[i]^2) over the grid-stride walk of a 256-thread workgroup, the n & 3 tail (workgroup 0) included.
// FLAG: `bad` additionally becomes 1 if any element this thread read is ±inf or NaN.
template <bool FLAG>
__device__ __forceinline__ double grad_sumsq_thread(const float* __restrict__ g, size_t n, unsigned& bad) {
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  // two float4 in flight per thread, as adam_kernel reads them
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const float4 a = ((const float4*)g)[i0];
    const float4 b = i1 < n4 ? ((const float4*)g)[i1] : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[0].x += a.x * a.x; acc[0].y += a.y * a.y; acc[0].z += a.z * a.z; acc[0].w += a.w * a.w;
    acc[1].x += b.x * b.x; acc[1].y += b.y * b.y; acc[1].z += b.z * b.z; acc[1].w += b.w * b.w;
    if (FLAG)
      bad |= nonfinite_bits(a.x) | nonfinite_bits(a.y) | nonfinite_bits(a.z) | nonfinite_bits(a.w) | nonfinite_bits(b.x) |
             nonfinite_bits(b.y) | nonfinite_bits(b.z) | nonfinite_bits(b.w);
  }
  double s = (((double)acc[0].x + (double)acc[0].y) + ((double)acc[0].z + (double)acc[0].w)) +
             (((double)acc[1].x + (double)acc[1].y) + ((double)acc[1].z + (double)acc[1].w));
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float t = g[(n4 << 2) + threadIdx.x];
    s += (double)(t * t);
    if (FLAG) bad |= nonfinite_bits(t);
  }
  return s;
}

// torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)); torch.clamp(max=1.0): a NaN norm gives a NaN coefficient
__device__ __forceinline__ float grad_clip_coef(double norm, float max_norm) {
  const double c = (double)max_norm / (norm + 1e-6);
  return (float)(c < 1.0 ? c : (c != c ? c : 1.0));
}

static inline int grad_clip_blocks(size_t n) { return grid_for(n >> 2, 512, CLIP_BLOCKS); }      // 512 float4 per workgroup and trip
