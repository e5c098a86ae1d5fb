// Small training-path kernels: gradient fork sums, mean-pool backward, token assembly, dropout (gfx950).
#include "common.h"

template <typename T>
__device__ inline float ld1(const void* p, size_t i, bool f32) {
  return f32 ? ((const float*)p)[i] : T::to_f32(((const uint16_t*)p)[i]);
}
template <typename T>
__device__ inline void st1(void* p, size_t i, bool f32, float v) {
  if (f32) ((float*)p)[i] = v;
  else ((uint16_t*)p)[i] = T::from_f32(v);
}

// y = a + b  (sum of the two gradients that meet at a fork), any mix of f32 / 16-bit
template <typename T>
__global__ void add_kernel(const void* __restrict__ a, const void* __restrict__ b, void* __restrict__ y, size_t n, int a_f32, int b_f32,
                           int y_f32) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    st1<T>(y, i, y_f32, ld1<T>(a, i, a_f32) + ld1<T>(b, i, b_f32));
}
extern "C" int vmc_add(const void* a, const void* b, void* y, size_t n, int a_dtype, int b_dtype, int y_dtype, int dtype16, void* stream) {
  if (!a || !b || !y || n == 0) return VMC_E_ARG;
  return dispatch16(dtype16, [&](auto t) {
    hipLaunchKernelGGL(add_kernel<decltype(t)>, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, n, a_dtype == VMC_F32,
                       b_dtype == VMC_F32, y_dtype == VMC_F32);
    return (int)hipGetLastError();
  });
}

// dx[b,t,:] = dout[b,:] / n on the n pooled rows, 0 on rows n..T-1   (backward of vmc_mean_pool_len; n = T without a pool length)
template <typename T>
__global__ void mean_pool_bwd_kernel(const void* __restrict__ dout, void* __restrict__ dx, int B, int Tn, int D, int do_f32, int dx_f32,
                                     const int* __restrict__ pool_len) {
  const size_t total = (size_t)B * Tn * D;
  const int np = pool_rows(pool_len, Tn);
  const float inv = 1.0f / (float)np;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / ((size_t)Tn * D);
    const int t = (int)((i / D) % Tn);
    const int d = (int)(i % D);
    st1<T>(dx, i, dx_f32, t < np ? ld1<T>(dout, b * D + d, do_f32) * inv : 0.f);
  }
}
extern "C" int vmc_mean_pool_bwd_len(const void* dout, void* dx, int B, int Tn, int D, const int* pool_len, int dout_dtype, int dx_dtype, int dtype16,
                                     void* stream) {
  if (!dout || !dx || B <= 0 || Tn <= 0 || D <= 0) return VMC_E_ARG;
  return dispatch16(dtype16, [&](auto t) {
    hipLaunchKernelGGL(mean_pool_bwd_kernel<decltype(t)>, dim3(grid_for((size_t)B * Tn * D, 256)), dim3(256), 0, (hipStream_t)stream, dout, dx, B,
                       Tn, D, dout_dtype == VMC_F32, dx_dtype == VMC_F32, pool_len);
    return (int)hipGetLastError();
  });
}
extern "C" int vmc_mean_pool_bwd(const void* dout, void* dx, int B, int Tn, int D, int dout_dtype, int dx_dtype, int dtype16, void* stream) {
  return vmc_mean_pool_bwd_len(dout, dx, B, Tn, D, nullptr, dout_dtype, dx_dtype, dtype16, stream);
}

// Token assembly (training path of K1): x[f,0,:] = cls + pos[0];  x[f,1+p,:] = xp[f*g2+p,:] + pos[1+p]
template <typename T>
__global__ void assemble_tokens_kernel(const uint16_t* __restrict__ xp, const float* __restrict__ cls, const float* __restrict__ pos,
                                       void* __restrict__ x, int F, int N, int D, int x_f32) {
  const size_t total = (size_t)F * N * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const int n = (int)((i / D) % N);
    const size_t f = i / ((size_t)N * D);
    const float v = (n == 0 ? cls[d] : T::to_f32(xp[(f * (N - 1) + (n - 1)) * D + d])) + pos[(size_t)n * D + d];
    st1<T>(x, i, x_f32, v);
  }
}
extern "C" int vmc_assemble_tokens(const void* xp, const float* cls, const float* pos, void* x, int F, int N, int D, int x_dtype,
                                   int dtype16, void* stream) {
  if (!xp || !cls || !pos || !x || F <= 0 || N <= 1 || D <= 0) return VMC_E_ARG;
  return dispatch16(dtype16, [&](auto t) {
    hipLaunchKernelGGL(assemble_tokens_kernel<decltype(t)>, dim3(grid_for((size_t)F * N * D, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)xp, cls, pos, x, F, N, D, x_dtype == VMC_F32);
    return (int)hipGetLastError();
  });
}

// Inverted dropout with a counter-based keep mask: keep(i) = hash(seed, i) >= p; y = x * keep / (1 - p).
// The backward calls the same function on dy with the same (seed, p): no mask is stored.
template <typename T>
__global__ void dropout_kernel(const void* __restrict__ x, void* __restrict__ y, size_t n, float p, uint64_t seed_arg, int f32) {
  const uint64_t seed = resolve_seed(seed_arg);
  const uint32_t thr = (uint32_t)((double)p * 4294967296.0);
  const float sc = 1.0f / (1.0f - p);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    st1<T>(y, i, f32, hash32(seed, i) >= thr ? ld1<T>(x, i, f32) * sc : 0.0f);
}
// 16-bit in / out, 8 elements (16 bytes) per thread and iteration: the scalar kernel above moves 2 B per lane and access
// (2 TB/s on a [8192, 2048] activation); same masks (hash of the element index).
template <typename T>
__global__ void __launch_bounds__(256) dropout16x8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, size_t n8, float p,
                                                          uint64_t seed_arg) {
  const uint64_t seed = resolve_seed(seed_arg);
  const uint32_t thr = (uint32_t)((double)p * 4294967296.0);
  const float sc = 1.0f / (1.0f - p);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 v = x[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a, b;
      unpack2<T>(w[j], a, b);
      a = hash32(seed, 8 * i + 2 * j) >= thr ? a * sc : 0.0f;
      b = hash32(seed, 8 * i + 2 * j + 1) >= thr ? b * sc : 0.0f;
      o[j] = pack2<T>(a, b);
    }
    y[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}
extern "C" int vmc_dropout(const void* x, void* y, size_t n, float p, uint64_t seed, int x_dtype, int dtype16, void* stream) {
  if (!x || !y || n == 0 || p < 0.f || p >= 1.f) return VMC_E_ARG;
  return dispatch16(dtype16, [&](auto t) {
    using T = decltype(t);
    if (x_dtype != VMC_F32 && (n & 7) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0)
      hipLaunchKernelGGL(dropout16x8_kernel<T>, dim3(grid_for(n / 8, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)y,
                         n / 8, p, seed);
    else
      hipLaunchKernelGGL(dropout_kernel<T>, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n, p, seed, x_dtype == VMC_F32);
    return (int)hipGetLastError();
  });
}

// y16 = cast(x32 * keep1/(1-p1) * keep2/(1-p2)): the gradient of a branch that went through one or two dropouts in front of a post-norm
// LayerNorm (vmc_postnorm_dropout_fwd), cast to the branch's 16-bit type in the same pass (was: a cast and one launch per dropout).
template <typename T>
__global__ void cast_dropout2_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, size_t n, float p1, uint64_t seed1_arg, float p2,
                                     uint64_t seed2_arg) {
  const uint64_t seed1 = p1 > 0.f ? resolve_seed(seed1_arg) : 0, seed2 = p2 > 0.f ? resolve_seed(seed2_arg) : 0;
  const uint32_t thr1 = (uint32_t)((double)p1 * 4294967296.0), thr2 = (uint32_t)((double)p2 * 4294967296.0);
  const float sc1 = 1.0f / (1.0f - p1), sc2 = 1.0f / (1.0f - p2);
  const size_t n8 = ((((uintptr_t)x | (uintptr_t)y) & 15) == 0) ? n / 8 : 0;      // 8 elements per thread while aligned, scalar tail
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = ((const float4*)x)[2 * i], b = ((const float4*)x)[2 * i + 1];
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (p1 > 0.f) v[j] = hash32(seed1, 8 * i + j) >= thr1 ? v[j] * sc1 : 0.0f;
      if (p2 > 0.f) v[j] = hash32(seed2, 8 * i + j) >= thr2 ? v[j] * sc2 : 0.0f;
    }
    ((uint4*)y)[i] = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
  }
  for (size_t i = 8 * n8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = x[i];
    if (p1 > 0.f) v = hash32(seed1, i) >= thr1 ? v * sc1 : 0.0f;
    if (p2 > 0.f) v = hash32(seed2, i) >= thr2 ? v * sc2 : 0.0f;
    y[i] = T::from_f32(v);
  }
}
extern "C" int vmc_cast_dropout2(const float* x, void* y16, size_t n, float p1, uint64_t seed1, float p2, uint64_t seed2, int dtype16,
                                 void* stream) {
  if (!x || !y16 || n == 0 || p1 < 0.f || p1 >= 1.f || p2 < 0.f || p2 >= 1.f) return VMC_E_ARG;
  return dispatch16(dtype16, [&](auto t) {
    hipLaunchKernelGGL(cast_dropout2_kernel<decltype(t)>, dim3(grid_for((n + 7) / 8, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream, x,
                       (uint16_t*)y16, n, p1, seed1, p2, seed2);
    return (int)hipGetLastError();
  });
}

// y = x * (*scale)   with the scale read from device memory (incoming scalar gradient of a loss)
__global__ void scale_dev_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n, const float* __restrict__ scale) {
  const float s = scale[0];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = x[i] * s;
}
extern "C" int vmc_scale_by_device_scalar(const float* x, float* y, size_t n, const float* scale, void* stream) {
  if (!x || !y || !scale || n == 0) return VMC_E_ARG;
  hipLaunchKernelGGL(scale_dev_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n, scale);
  VMC_CHECK_LAUNCH();
  return 0;
}


// ---- sustained shader clock under an MFMA load (diagnostics: bench.py `clock_probe`) -----------------------------------------
// One 256-thread workgroup per CU runs `iters` rounds of 64 dependent-free bf16 MFMAs on pseudo-random operands and stamps
// s_memtime (shader cycles) and s_memrealtime (100 MHz) around them: cycles / ticks x 100 MHz = the clock the chip holds under
// that load (MI355X_MICROARCH.md, DVFS give-back item 6).  The stamps go to `out` only; nothing else reads them.
// mode 0: v_mfma_f32_16x16x32_bf16, mode 1: v_mfma_f32_32x32x16_bf16 (same FLOPs per cycle; which clock does the chip hold?)
__global__ void __launch_bounds__(256) clock_probe32_kernel(unsigned long long* __restrict__ out, int iters) {
  const unsigned seed = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
  uint4 a, b;
  a.x = 0x3F803F80u ^ (seed & 0x007F007Fu); a.y = 0x3F003F80u ^ ((seed >> 3) & 0x007F007Fu);
  a.z = 0xBF803F00u ^ ((seed >> 5) & 0x007F007Fu); a.w = 0x3F80BF80u ^ ((seed >> 7) & 0x007F007Fu);
  b.x = a.y ^ 0x00110011u; b.y = a.z ^ 0x00220022u; b.z = a.w ^ 0x00330033u; b.w = a.x ^ 0x00440044u;
  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc[i], 0, 0, 0);
    a.x ^= (unsigned)it;
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float sink = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) sink += acc[i][e];
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = c1 - c0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
  if (sink == 12345.678f) out[0] = 0;
}
__global__ void __launch_bounds__(256) clock_probe_kernel(unsigned long long* __restrict__ out, int iters) {
  const unsigned seed = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
  uint4 a, b;
  a.x = 0x3F803F80u ^ (seed & 0x007F007Fu); a.y = 0x3F003F80u ^ ((seed >> 3) & 0x007F007Fu);
  a.z = 0xBF803F00u ^ ((seed >> 5) & 0x007F007Fu); a.w = 0x3F80BF80u ^ ((seed >> 7) & 0x007F007Fu);
  b.x = a.y ^ 0x00110011u; b.y = a.z ^ 0x00220022u; b.z = a.w ^ 0x00330033u; b.w = a.x ^ 0x00440044u;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = BF16::mfma16(a, b, acc[i]);
    a.x ^= (unsigned)it;
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float sink = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) sink += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = c1 - c0;
    out[2 * blockIdx.x + 1] = r1 - r0;
  }
  if (sink == 12345.678f) out[0] = 0;      // keeps the MFMAs alive
}
extern "C" int vmc_clock_probe(void* out, int workgroups, int iters, int mfma_shape, void* stream) {
  if (!out || workgroups <= 0 || iters <= 0 || mfma_shape < 0 || mfma_shape > 1) return VMC_E_ARG;
  if (mfma_shape == 1)      // 32 MFMAs of 32x32x16 per round = the FLOPs of 64 MFMAs of 16x16x32
    hipLaunchKernelGGL(clock_probe32_kernel, dim3(workgroups), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)out, iters);
  else
    hipLaunchKernelGGL(clock_probe_kernel, dim3(workgroups), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)out, iters);
  VMC_CHECK_LAUNCH();
  return 0;
}
