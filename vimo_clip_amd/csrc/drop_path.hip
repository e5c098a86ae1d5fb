// Stochastic depth that skips dropped frames, in the student's training tower: draw the frames a block keeps, gather
// their rows in front of the block, merge the block's output back into the stream, and the backward of both (gfx950).  All five are
// memory-bound row movers around the unchanged block; no floating-point atomics anywhere: every call gives the same bits.
#include "common.h"

// ---- W consecutive elements of a row.  F32: float, else the 16-bit type T.  VEC: one 16-byte access (4 floats / 8 halves), else one element.
template <bool F32, bool VEC>
struct DpWidth { static constexpr int W = VEC ? (F32 ? 4 : 8) : 1; };

template <typename T, bool F32, bool VEC>
__device__ inline void dp_ld(const void* p, size_t i, float (&v)[DpWidth<F32, VEC>::W]) {
  if constexpr (VEC && F32) {
    const float4 a = *(const float4*)((const float*)p + i);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else if constexpr (VEC) {
    const uint4 u = *(const uint4*)((const uint16_t*)p + i);
    unpack2<T>(u.x, v[0], v[1]); unpack2<T>(u.y, v[2], v[3]); unpack2<T>(u.z, v[4], v[5]); unpack2<T>(u.w, v[6], v[7]);
  } else if constexpr (F32) {
    v[0] = ((const float*)p)[i];
  } else {
    v[0] = T::to_f32(((const uint16_t*)p)[i]);
  }
}
template <typename T, bool F32, bool VEC>
__device__ inline void dp_st(void* p, size_t i, const float (&v)[DpWidth<F32, VEC>::W]) {
  if constexpr (VEC && F32) {
    *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (VEC) {
    *(uint4*)((uint16_t*)p + i) = make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7]));
  } else if constexpr (F32) {
    ((float*)p)[i] = v[0];
  } else {
    ((uint16_t*)p)[i] = T::from_f32(v[0]);
  }
}
// W elements moved as bits: what a dropped row, a gathered row and an unscaled gradient row are
template <bool F32, bool VEC>
__device__ inline void dp_copy(const void* src, size_t i, void* dst, size_t o) {
  if constexpr (VEC) *(uint4*)((char*)dst + o * (F32 ? 4 : 2)) = *(const uint4*)((const char*)src + i * (F32 ? 4 : 2));
  else if constexpr (F32) ((uint32_t*)dst)[o] = ((const uint32_t*)src)[i];
  else ((uint16_t*)dst)[o] = ((const uint16_t*)src)[i];
}
static inline bool dp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// a pointer that is not a multiple of its element size cannot be read even element by element
template <typename... P>
static inline bool dp_misaligned(int eb, P... ptrs) {
  for (const void* p : {(const void*)ptrs...})
    if ((uintptr_t)p % (uintptr_t)eb) return true;
  return false;
}
static inline int dp_elem_bytes(int dtype) { return dtype == VMC_F32 ? 4 : ((dtype == VMC_BF16 || dtype == VMC_F16) ? 2 : 0); }
// A frame id read from device memory, which the host cannot validate: clamped into [0, F-1] so that no row outside the arrays is touched.
__device__ inline size_t dp_frame_id(const int* __restrict__ keep, size_t j, int F) {
  const int f = keep[j];
  return (size_t)(f < 0 ? 0 : (f >= F ? F - 1 : f));
}

// launch `kernel<T, F32, VEC>` for the dtype: f32 rows need no 16-bit type (BF16 stands in, unused)
#define DP_LAUNCH(kernel, dtype, vec, items, stream, ...)                                                                      \
  do {                                                                                                                         \
    const dim3 grid_(grid_for((items), 256, 256 * 32)), block_(256);                                                           \
    if ((dtype) == VMC_F32) {                                                                                                  \
      if (vec) hipLaunchKernelGGL((kernel<BF16, true, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);           \
      else hipLaunchKernelGGL((kernel<BF16, true, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);              \
    } else if ((dtype) == VMC_BF16) {                                                                                          \
      if (vec) hipLaunchKernelGGL((kernel<BF16, false, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);          \
      else hipLaunchKernelGGL((kernel<BF16, false, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);             \
    } else {                                                                                                                   \
      if (vec) hipLaunchKernelGGL((kernel<F16, false, true>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);           \
      else hipLaunchKernelGGL((kernel<F16, false, false>), grid_, block_, 0, (hipStream_t)(stream), __VA_ARGS__);              \
    }                                                                                                                          \
  } while (0)

// ---- keep-set sampler: one workgroup, keys in LDS, rank by counting, compaction in ascending frame id ------------------------------
#define DP_MAX_F 8192
#define DP_THREADS 1024
__global__ void __launch_bounds__(DP_THREADS) drop_path_sample_kernel(uint64_t seed_arg, int block, int F, int K, int* __restrict__ keep,
                                                                      int* __restrict__ slot) {
  __shared__ uint32_t key[DP_MAX_F];
  __shared__ uint8_t kept[DP_MAX_F];
  __shared__ int cnt[DP_THREADS];
  const uint64_t seed = resolve_seed(seed_arg);
  const int tid = threadIdx.x;
  for (int f = tid; f < F; f += DP_THREADS) key[f] = hash32(seed, (uint64_t)block * F + f);
  __syncthreads();
  for (int n = tid; n < F; n += DP_THREADS) {
    const uint32_t kn = key[n];
    int rank = 0;                                        // frames in front of n in the strict total order (key, id)
    for (int m = 0; m < F; ++m) {
      const uint32_t km = key[m];                        // one address per wave: an LDS broadcast
      rank += (km < kn || (km == kn && m < n)) ? 1 : 0;
    }
    kept[n] = rank < K;                                  // the ranks are a permutation of 0..F-1: exactly K frames are kept
  }
  __syncthreads();
  // compaction: thread t owns the frames [t chunk, (t + 1) chunk); its first kept frame lands behind the kept frames of the threads before it
  const int chunk = (F + DP_THREADS - 1) / DP_THREADS;
  const int lo = tid * chunk < F ? tid * chunk : F, hi = lo + chunk < F ? lo + chunk : F;
  int mine = 0;
  for (int n = lo; n < hi; ++n) mine += kept[n];
  cnt[tid] = mine;
  __syncthreads();
  int pos = 0;
  for (int t = 0; t < tid; ++t) pos += cnt[t];
  for (int n = lo; n < hi; ++n) {
    if (kept[n]) {
      keep[pos] = n;                                     // pos < K: fewer than K kept frames lie in front of a kept one
      slot[n] = pos++;
    } else {
      slot[n] = -1;
    }
  }
}
extern "C" int vmc_drop_path_sample(uint64_t seed, int block, int F, int K, int* keep, int* slot, void* stream) {
  if (!keep || !slot || block < 0) return VMC_E_ARG;
  if (K < 1 || K > F || F > DP_MAX_F) return VMC_E_SHAPE;
  hipLaunchKernelGGL(drop_path_sample_kernel, dim3(1), dim3(DP_THREADS), 0, (hipStream_t)stream, seed, block, F, K, keep, slot);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- dst[j, :] = src[keep[j], :]: bit copies ----------------------------------------------------------------------------------------
template <typename T, bool F32, bool VEC>
__global__ void __launch_bounds__(256) frame_gather_kernel(const void* __restrict__ src, const int* __restrict__ keep, void* __restrict__ dst,
                                                           int F, int K, size_t row) {
  constexpr int W = DpWidth<F32, VEC>::W;
  const size_t rw = row / W, total = (size_t)K * rw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t j = i / rw, c = (i % rw) * W;
    dp_copy<F32, VEC>(src, dp_frame_id(keep, j, F) * row + c, dst, j * row + c);
  }
}
extern "C" int vmc_frame_gather(const void* src, const int* keep, void* dst, int F, int K, size_t row, int dtype, void* stream) {
  if (!src || !keep || !dst || row == 0) return VMC_E_ARG;
  if (K < 1 || K > F) return VMC_E_SHAPE;
  const int eb = dp_elem_bytes(dtype);
  if (eb == 0) return VMC_E_DTYPE;
  if (dp_misaligned(eb, src, dst)) return VMC_E_ALIGN;
  const bool vec = row % (16 / eb) == 0 && dp_aligned16(src) && dp_aligned16(dst);
  DP_LAUNCH(frame_gather_kernel, dtype, vec, (size_t)K * (vec ? row / (16 / eb) : row), stream, src, keep, dst, F, K, row);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- dx[f, :] = dpass[f, :] + (slot[f] >= 0 ? dsub[slot[f], :] : 0): the backward of a gather that also passes its input on ---------
template <typename T, bool F32, bool VEC>
__global__ void __launch_bounds__(256) frame_scatter_add_kernel(const void* __restrict__ dpass, const void* __restrict__ dsub,
                                                                const int* __restrict__ slot, void* __restrict__ dx, int F, size_t row) {
  constexpr int W = DpWidth<F32, VEC>::W;
  const size_t rw = row / W, total = (size_t)F * rw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t f = i / rw, c = (i % rw) * W;
    const int j = slot[f];
    if (j < 0) {
      dp_copy<F32, VEC>(dpass, f * row + c, dx, f * row + c);
      continue;
    }
    float a[W], b[W];
    dp_ld<T, F32, VEC>(dpass, f * row + c, a);
    dp_ld<T, F32, VEC>(dsub, (size_t)(j < F ? j : F - 1) * row + c, b);      // j < K <= F for a slot array that inverts a keep set
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] += b[e];
    dp_st<T, F32, VEC>(dx, f * row + c, a);
  }
}
extern "C" int vmc_frame_scatter_add(const void* dpass, const void* dsub, const int* slot, void* dx, int F, size_t row, int dtype,
                                     void* stream) {
  if (!dpass || !dsub || !slot || !dx || row == 0) return VMC_E_ARG;
  if (F < 1) return VMC_E_SHAPE;
  const int eb = dp_elem_bytes(dtype);
  if (eb == 0) return VMC_E_DTYPE;
  if (dp_misaligned(eb, dpass, dsub, dx)) return VMC_E_ALIGN;
  const bool vec = row % (16 / eb) == 0 && dp_aligned16(dpass) && dp_aligned16(dsub) && dp_aligned16(dx);
  DP_LAUNCH(frame_scatter_add_kernel, dtype, vec, (size_t)F * (vec ? row / (16 / eb) : row), stream, dpass, dsub, slot, dx, F, row);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- out[f, :] = slot[f] >= 0 ? c x[f, :] + s y[slot[f], :] : x[f, :] ---------------------------------------------------------------
template <typename T, bool F32, bool VEC>
__global__ void __launch_bounds__(256) drop_path_merge_kernel(const void* __restrict__ x, const void* __restrict__ y,
                                                              const int* __restrict__ slot, void* __restrict__ out, int F, size_t row,
                                                              float cx, float sy) {
#pragma clang fp contract(off)      // two products and one sum, each rounded: the bits do not depend on what the compiler fuses
  constexpr int W = DpWidth<F32, VEC>::W;
  const size_t rw = row / W, total = (size_t)F * rw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t f = i / rw, c = (i % rw) * W;
    const int j = slot[f];
    if (j < 0) {
      dp_copy<F32, VEC>(x, f * row + c, out, f * row + c);
      continue;
    }
    float a[W], b[W];
    dp_ld<T, F32, VEC>(x, f * row + c, a);
    dp_ld<T, F32, VEC>(y, (size_t)(j < F ? j : F - 1) * row + c, b);
#pragma unroll
    for (int e = 0; e < W; ++e) a[e] = cx * a[e] + sy * b[e];
    dp_st<T, F32, VEC>(out, f * row + c, a);
  }
}
extern "C" int vmc_drop_path_merge(const void* x, const void* y, const int* slot, void* out, int F, size_t row, float c, float s, int dtype,
                                   void* stream) {
  if (!x || !y || !slot || !out || row == 0) return VMC_E_ARG;
  if (F < 1) return VMC_E_SHAPE;
  const int eb = dp_elem_bytes(dtype);
  if (eb == 0) return VMC_E_DTYPE;
  if (dp_misaligned(eb, x, y, out)) return VMC_E_ALIGN;
  const bool vec = row % (16 / eb) == 0 && dp_aligned16(x) && dp_aligned16(y) && dp_aligned16(out);
  DP_LAUNCH(drop_path_merge_kernel, dtype, vec, (size_t)F * (vec ? row / (16 / eb) : row), stream, x, y, slot, out, F, row, c, s);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- dx[f, :] = slot[f] >= 0 ? c dout[f, :] : dout[f, :];  dy[j, :] = s dout[keep[j], :]: rows 0..F-1 of the launch are dx, F..F+K-1 dy
template <typename T, bool F32, bool VEC>
__global__ void __launch_bounds__(256) drop_path_merge_bwd_kernel(const void* __restrict__ dout, const int* __restrict__ keep,
                                                                  const int* __restrict__ slot, void* __restrict__ dx,
                                                                  void* __restrict__ dy, int F, int K, size_t row, float cx, float sy) {
  constexpr int W = DpWidth<F32, VEC>::W;
  const size_t rw = row / W, total = ((size_t)F + K) * rw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / rw, c = (i % rw) * W;
    float a[W];
    if (r < (size_t)F) {
      if (slot[r] < 0) {
        dp_copy<F32, VEC>(dout, r * row + c, dx, r * row + c);
        continue;
      }
      dp_ld<T, F32, VEC>(dout, r * row + c, a);
#pragma unroll
      for (int e = 0; e < W; ++e) a[e] *= cx;
      dp_st<T, F32, VEC>(dx, r * row + c, a);
    } else {
      const size_t j = r - F;
      dp_ld<T, F32, VEC>(dout, dp_frame_id(keep, j, F) * row + c, a);
#pragma unroll
      for (int e = 0; e < W; ++e) a[e] *= sy;
      dp_st<T, F32, VEC>(dy, j * row + c, a);
    }
  }
}
extern "C" int vmc_drop_path_merge_bwd(const void* dout, const int* keep, const int* slot, void* dx, void* dy, int F, int K, size_t row,
                                       float c, float s, int dtype, void* stream) {
  if (!dout || !keep || !slot || !dx || !dy || row == 0) return VMC_E_ARG;
  if (K < 1 || K > F) return VMC_E_SHAPE;
  const int eb = dp_elem_bytes(dtype);
  if (eb == 0) return VMC_E_DTYPE;
  if (dp_misaligned(eb, dout, dx, dy)) return VMC_E_ALIGN;
  const bool vec = row % (16 / eb) == 0 && dp_aligned16(dout) && dp_aligned16(dx) && dp_aligned16(dy);
  DP_LAUNCH(drop_path_merge_bwd_kernel, dtype, vec, ((size_t)F + K) * (vec ? row / (16 / eb) : row), stream, dout, keep, slot, dx, dy, F,
            K, row, c, s);
  VMC_CHECK_LAUNCH();
  return 0;
}
