// Patch dropout in the student's training stem: draw a keep set per frame, gather the kept patch rows in front of
// the conv1 GEMM, assemble tokens with a per-frame gather of the positional embedding, and the backward of that assembly (gfx950).
// All four are memory-bound row movers; no floating-point atomics anywhere: every sum has an order fixed by the shape and `keep`.
#include "common.h"

// ---- W consecutive elements of a row, f32 or 16-bit.  W = 8: one 16-byte access per 16-bit row piece (two for f32); W = 1: scalar.
template <typename T, int W>
__device__ inline void ld_w(const void* p, size_t i, bool f32, float (&v)[W]) {
  if constexpr (W == 8) {
    if (f32) {
      const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
      const uint4 u = *(const uint4*)((const uint16_t*)p + i);
      unpack2<T>(u.x, v[0], v[1]); unpack2<T>(u.y, v[2], v[3]); unpack2<T>(u.z, v[4], v[5]); unpack2<T>(u.w, v[6], v[7]);
    }
  } else {
    v[0] = f32 ? ((const float*)p)[i] : T::to_f32(((const uint16_t*)p)[i]);
  }
}
template <typename T, int W>
__device__ inline void st_w(void* p, size_t i, bool f32, const float (&v)[W]) {
  if constexpr (W == 8) {
    if (f32) {
      *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)((float*)p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      *(uint4*)((uint16_t*)p + i) = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
    }
  } else {
    if (f32) ((float*)p)[i] = v[0];
    else ((uint16_t*)p)[i] = T::from_f32(v[0]);
  }
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// A patch id read from device memory, which the host cannot validate: clamped into [0, G-1] so that no row outside the arrays is touched.
__device__ inline int patch_id(const int* __restrict__ keep, size_t i, int G) {
  const int n = keep[i];
  return n < 0 ? 0 : (n >= G ? G - 1 : n);
}

// ---- keep-set sampler: one workgroup per frame, keys in LDS, rank by counting, compaction in ascending patch id -------------------
#define PD_MAX_G 1024
__global__ void __launch_bounds__(256) patch_keep_sample_kernel(uint64_t seed_arg, int G, int Kp, int* __restrict__ keep) {
  __shared__ uint32_t key[PD_MAX_G];
  __shared__ uint8_t kept[PD_MAX_G];
  const uint64_t seed = resolve_seed(seed_arg);
  const int f = blockIdx.x;
  for (int n = threadIdx.x; n < G; n += 256) key[n] = hash32(seed, (uint64_t)f * G + n);
  __syncthreads();
  for (int n = threadIdx.x; n < G; n += 256) {
    const uint32_t kn = key[n];
    int rank = 0;                                        // patches in front of n in the strict total order (key, id)
    for (int m = 0; m < G; ++m) {
      const uint32_t km = key[m];
      rank += (km < kn || (km == kn && m < n)) ? 1 : 0;
    }
    kept[n] = rank < Kp;                                 // the ranks are a permutation of 0..G-1: exactly Kp patches are kept
  }
  __syncthreads();
  for (int n = threadIdx.x; n < G; n += 256) {
    if (!kept[n]) continue;
    int pos = 0;
    for (int m = 0; m < n; ++m) pos += kept[m];
    keep[(size_t)f * Kp + pos] = n;                      // pos < Kp: fewer than Kp kept patches lie in front of a kept one
  }
}
extern "C" int vmc_patch_keep_sample(uint64_t seed, int F, int G, int Kp, int* keep, void* stream) {
  if (!keep || F <= 0) return VMC_E_ARG;
  if (Kp < 1 || Kp > G || G > PD_MAX_G) return VMC_E_SHAPE;
  hipLaunchKernelGGL(patch_keep_sample_kernel, dim3(F), dim3(256), 0, (hipStream_t)stream, seed, G, Kp, keep);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- dst[f Kp + j] = src[f G + idx[f, j]]: bit copies of 16-bit rows ----------------------------------------------------------------
template <typename V>      // uint4: 8 elements per access; uint16_t: one
__global__ void __launch_bounds__(256) gather_rows16_kernel(const uint16_t* __restrict__ src, size_t ld_src, const int* __restrict__ idx, int G,
                                                            uint16_t* __restrict__ dst, size_t ld_dst, int cols, int F, int Kp) {
  constexpr int W = sizeof(V) / 2;
  const int cw = cols / W;
  const size_t total = (size_t)F * Kp * cw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % cw) * W;
    const size_t r = i / cw;                             // f Kp + j
    const size_t f = r / Kp;
    const size_t s = f * G + patch_id(idx, r, G);
    *(V*)(dst + r * ld_dst + c) = *(const V*)(src + s * ld_src + c);
  }
}
extern "C" int vmc_gather_rows16(const void* src, int ld_src, const int* idx, int G, void* dst, int ld_dst, int cols, int F, int Kp,
                                 void* stream) {
  if (!src || !idx || !dst || F <= 0 || cols <= 0) return VMC_E_ARG;
  if (Kp < 1 || Kp > G || ld_src < cols || ld_dst < cols) return VMC_E_SHAPE;
  const bool vec = cols % 8 == 0 && ld_src % 8 == 0 && ld_dst % 8 == 0 && aligned16(src) && aligned16(dst);
  const size_t items = (size_t)F * Kp * (vec ? cols / 8 : cols);
  if (vec)
    hipLaunchKernelGGL(gather_rows16_kernel<uint4>, dim3(grid_for(items, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)src, (size_t)ld_src, idx, G, (uint16_t*)dst, (size_t)ld_dst, cols, F, Kp);
  else
    hipLaunchKernelGGL(gather_rows16_kernel<uint16_t>, dim3(grid_for(items, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)src, (size_t)ld_src, idx, G, (uint16_t*)dst, (size_t)ld_dst, cols, F, Kp);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- token assembly on the kept patches: x[f, 0] = cls + pos[0];  x[f, 1 + j] = xp[f Kp + j] + pos[keep[f, j] + 1] ----------------
// The arithmetic of assemble_tokens_kernel (glue.hip): one fp32 add, then the store rounding of the residual type.
template <typename T, int W>
__global__ void __launch_bounds__(256) assemble_tokens_keep_kernel(const uint16_t* __restrict__ xp, const float* __restrict__ cls,
                                                                   const float* __restrict__ pos, const int* __restrict__ keep,
                                                                   void* __restrict__ x, int F, int G, int Kp, int D, int x_f32) {
  const int dw = D / W, N = Kp + 1;
  const size_t total = (size_t)F * N * dw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % dw) * W;
    const size_t r = i / dw;                             // f N + t
    const int t = (int)(r % N);
    const size_t f = r / N;
    float a[W], b[W];
    if (t == 0) {
      ld_w<T, W>(cls, d, true, a);
      ld_w<T, W>(pos, d, true, b);
    } else {
      const size_t j = f * Kp + (t - 1);
      ld_w<T, W>(xp, j * D + d, false, a);
      ld_w<T, W>(pos, (size_t)(patch_id(keep, j, G) + 1) * D + d, true, b);
    }
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] += b[e];
    st_w<T, W>(x, r * D + d, x_f32, a);
  }
}
extern "C" int vmc_assemble_tokens_keep(const void* xp, const float* cls, const float* pos, const int* keep, void* x, int F, int G, int Kp,
                                        int D, int x_dtype, int dtype16, void* stream) {
  if (!xp || !cls || !pos || !keep || !x || F <= 0 || D <= 0) return VMC_E_ARG;
  if (Kp < 1 || Kp > G) return VMC_E_SHAPE;
  if (x_dtype != VMC_F32 && x_dtype != dtype16) return VMC_E_DTYPE;
  const bool vec = D % 8 == 0 && aligned16(xp) && aligned16(cls) && aligned16(pos) && aligned16(x);
  const size_t items = (size_t)F * (Kp + 1) * (vec ? D / 8 : D);
  return dispatch16(dtype16, [&](auto t) {
    using T = decltype(t);
    if (vec)
      hipLaunchKernelGGL((assemble_tokens_keep_kernel<T, 8>), dim3(grid_for(items, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                         (const uint16_t*)xp, cls, pos, keep, x, F, G, Kp, D, x_dtype == VMC_F32);
    else
      hipLaunchKernelGGL((assemble_tokens_keep_kernel<T, 1>), dim3(grid_for(items, 256, 256 * 32)), dim3(256), 0, (hipStream_t)stream,
                         (const uint16_t*)xp, cls, pos, keep, x, F, G, Kp, D, x_dtype == VMC_F32);
    return (int)hipGetLastError();
  });
}

// ---- backward of the assembly ------------------------------------------------------------------------------------------------------
// Three launches.  (1) slot[f, n] = j where keep[f, j] = n, -1 where frame f dropped patch n (the inverse of keep, in the workspace).
// (2) dxp = round16(dx patch rows), a row mover.  (3) one thread per (position, 8 columns, slab of frames) walks its frames in
// ascending order and adds dx[f, slot] where the frame kept the position: fp32, order fixed by (F, keep).  With more than one slab the
// partial sums go to the workspace and (4) adds them in slab order.  dcls is dpos[0].
#define PD_SLAB_FRAMES 64
#define PD_MAX_SLABS 8
static int pd_slabs(int F) { int s = F / PD_SLAB_FRAMES; return s < 1 ? 1 : (s > PD_MAX_SLABS ? PD_MAX_SLABS : s); }
static size_t pd_slot_bytes(int F, int G) { return ((size_t)F * G * sizeof(int) + 15) & ~(size_t)15; }
extern "C" size_t vmc_assemble_tokens_keep_bwd_workspace_bytes(int F, int G, int D) {
  if (F <= 0 || G <= 0 || D <= 0) return 0;
  const int S = pd_slabs(F);
  return pd_slot_bytes(F, G) + (S > 1 ? (size_t)S * (G + 1) * D * sizeof(float) : 0);
}

__global__ void __launch_bounds__(256) keep_slots_kernel(const int* __restrict__ keep, int* __restrict__ slot, int G, int Kp) {
  const size_t f = blockIdx.x;
  for (int n = threadIdx.x; n < G; n += 256) slot[f * G + n] = -1;
  __syncthreads();
  for (int j = threadIdx.x; j < Kp; j += 256) {
    const int n = keep[f * Kp + j];
    if (n >= 0 && n < G) slot[f * G + n] = j;
  }
}

template <typename T, int W>
__global__ void __launch_bounds__(256) keep_dxp_kernel(const void* __restrict__ dx, void* __restrict__ dxp, int F, int Kp, int D, int dx_f32) {
  const int dw = D / W;
  const size_t total = (size_t)F * Kp * dw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % dw) * W;
    const size_t r = i / dw;                             // f Kp + j
    const size_t f = r / Kp;
    float v[W];
    ld_w<T, W>(dx, (r + f + 1) * D + d, dx_f32, v);      // row f (Kp + 1) + 1 + j
    st_w<T, W>(dxp, r * D + d, false, v);
  }
}

template <typename T, int W>
__global__ void __launch_bounds__(256) keep_dpos_kernel(const void* __restrict__ dx, const int* __restrict__ slot, float* __restrict__ out,
                                                        float* __restrict__ dcls, int F, int G, int Kp, int D, int dx_f32, int slabs) {
  const int dw = D / W, N = Kp + 1;
  const size_t per_slab = (size_t)(G + 1) * dw;
  const int s = blockIdx.y;
  const int f0 = (int)((long long)F * s / slabs), f1 = (int)((long long)F * (s + 1) / slabs);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_slab; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % dw) * W;
    const int n = (int)(i / dw);                         // position 0 = class token, n = patch n - 1
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    for (int f = f0; f < f1; ++f) {
      const int j = n == 0 ? 0 : slot[(size_t)f * G + (n - 1)] + 1;      // token row inside the frame; 0 for a dropped patch
      if (n != 0 && j == 0) continue;
      float v[W];
      ld_w<T, W>(dx, ((size_t)f * N + j) * D + d, dx_f32, v);
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] += v[e];
    }
    st_w<T, W>(out, ((size_t)s * (G + 1) + n) * D + d, true, acc);
    if (dcls != nullptr && n == 0) st_w<T, W>(dcls, d, true, acc);      // one slab: the sums are final
  }
}

// dpos = sum of the slabs in slab order; dcls = dpos[0]
__global__ void __launch_bounds__(256) keep_dpos_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dpos,
                                                               float* __restrict__ dcls, size_t n, int D, int slabs) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float acc = partial[i];
    for (int s = 1; s < slabs; ++s) acc += partial[(size_t)s * n + i];
    dpos[i] = acc;
    if (i < (size_t)D) dcls[i] = acc;
  }
}

extern "C" int vmc_assemble_tokens_keep_bwd(const void* dx, const int* keep, void* dxp16, float* dcls, float* dpos, int F, int G, int Kp,
                                            int D, int dx_dtype, int dtype16, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dx || !keep || !dxp16 || !dcls || !dpos || !workspace || F <= 0 || D <= 0) return VMC_E_ARG;
  if (Kp < 1 || Kp > G) return VMC_E_SHAPE;
  if (workspace_bytes < vmc_assemble_tokens_keep_bwd_workspace_bytes(F, G, D)) return VMC_E_ARG;
  if (!aligned16(workspace)) return VMC_E_ALIGN;
  if (dx_dtype != VMC_F32 && dx_dtype != dtype16) return VMC_E_DTYPE;
  hipStream_t s = (hipStream_t)stream;
  const int S = pd_slabs(F);
  int* slot = (int*)workspace;
  float* partial = (float*)((char*)workspace + pd_slot_bytes(F, G));
  const bool vec = D % 8 == 0 && aligned16(dx) && aligned16(dxp16) && aligned16(dpos) && aligned16(dcls);
  const int dx_f32 = dx_dtype == VMC_F32;
  return dispatch16(dtype16, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(keep_slots_kernel, dim3(F), dim3(256), 0, s, keep, slot, G, Kp);
    const size_t row_items = (size_t)F * Kp * (vec ? D / 8 : D), pos_items = (size_t)(G + 1) * (vec ? D / 8 : D);
    float* out = S > 1 ? partial : dpos;
    const dim3 pos_grid(grid_for(pos_items, 256), S);
    if (vec) {
      hipLaunchKernelGGL((keep_dxp_kernel<T, 8>), dim3(grid_for(row_items, 256, 256 * 32)), dim3(256), 0, s, dx, dxp16, F, Kp, D, dx_f32);
      hipLaunchKernelGGL((keep_dpos_kernel<T, 8>), pos_grid, dim3(256), 0, s, dx, slot, out, S > 1 ? nullptr : dcls, F, G, Kp, D, dx_f32, S);
    } else {
      hipLaunchKernelGGL((keep_dxp_kernel<T, 1>), dim3(grid_for(row_items, 256, 256 * 32)), dim3(256), 0, s, dx, dxp16, F, Kp, D, dx_f32);
      hipLaunchKernelGGL((keep_dpos_kernel<T, 1>), pos_grid, dim3(256), 0, s, dx, slot, out, S > 1 ? nullptr : dcls, F, G, Kp, D, dx_f32, S);
    }
    if (S > 1)
      hipLaunchKernelGGL(keep_dpos_reduce_kernel, dim3(grid_for((size_t)(G + 1) * D, 256)), dim3(256), 0, s, partial, dpos, dcls,
                         (size_t)(G + 1) * D, D, S);
    return (int)hipGetLastError();
  });
}
