// Row LayerNorm in the wave-per-row layout: a lane holds float4 chunk c of the row at columns c * 256 + lane * 4.  The one body
// behind ln_fwd_kernel, add_ln_kernel, postnorm_kernel (layernorm.hip) and both LayerNorms of tf_pool_kernel (tfam_kernels.h): the
// float64-reference tests pin the order of these additions, so it is written once.  Each kernel keeps its loads, adds and stores,
// and the chunk loop in which it adds up ln_chunk_sum.
#pragma once
#include <type_traits>

#include "common.h"

// FULL says whether the row is exactly 256 N wide (D is not read) or D is a run-time width with chunks at col >= D left out (they
// may be uninitialised).  It is a template constant, so a full row carries no guard at all.
template <bool FULL, int N>
__device__ __forceinline__ float ln_row_inv_width(int D) {
  if constexpr (FULL) return 1.0f / (N * 256);
  else return 1.0f / (float)D;
}

// A lane's share of the row sum from one chunk.  Each kernel adds it up in its own chunk loop, beside that chunk's adds and stores:
// gathered in one block, the N sums are packed across chunks by the SLP vectoriser, which costs registers (add_ln_kernel<*, 3>: a
// wave of occupancy) and moves which product of p * p + q * q below is fused.
__device__ __forceinline__ float ln_chunk_sum(float4 v) { return (v.x + v.y) + (v.z + v.w); }

// mean of the row from the lane's sum s of ln_chunk_sum over its chunks, in chunk order
template <bool FULL, int N>
__device__ __forceinline__ float ln_row_mean(float s, int D) {
  return wave_sum(s) * ln_row_inv_width<FULL, N>(D);
}

// rstd of the row whose chunks are v[0..N)
template <bool FULL, int N>
__device__ __forceinline__ float ln_row_rstd(const float4 (&v)[N], int lane, int D, float mean, float eps) {
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    bool counts = true;
    if constexpr (!FULL) counts = c * 256 + lane * 4 < D;
    if (counts) {
      const float p = v[c].x - mean, q = v[c].y - mean, r = v[c].z - mean, t = v[c].w - mean;
      ss += (p * p + q * q) + (r * r + t * t);
    }
  }
  return rsqrtf(wave_sum(ss) * ln_row_inv_width<FULL, N>(D) + eps);
}

// the normalised, scaled and shifted chunk
__device__ __forceinline__ float4 ln_row_affine(float4 v, float mean, float rstd, float4 g, float4 b) {
  return make_float4((v.x - mean) * rstd * g.x + b.x, (v.y - mean) * rstd * g.y + b.y, (v.z - mean) * rstd * g.z + b.z,
                     (v.w - mean) * rstd * g.w + b.w);
}

// The float4 chunks per lane of a launch, as a type: the launchers pick the kernel instantiation from the run-time D with it.
template <int N>
using chunks = std::integral_constant<int, N>;

// Full rows: f(chunks<D / 256>) for D = 256 .. 2048 in steps of 256; false (f not called) for any other D.
template <int... N, typename F>
static inline bool ln_chunks_among(int D, F&& f) { return ((D == 256 * N && (f(chunks<N>{}), true)) || ...); }
template <typename F>
static inline bool ln_chunks_exact(int D, F&& f) { return ln_chunks_among<1, 2, 3, 4, 5, 6, 7, 8>(D, f); }

// Guarded rows: f(the smallest of 2, 3, 4, 8 .. MAXCH chunks that holds D), MAXCH = 8 or 16; the caller has checked D <= 256 MAXCH.
template <int MAXCH, typename F>
static inline void ln_chunks_ceil(int D, F&& f) {
  static_assert(MAXCH == 8 || MAXCH == 16, "the ladder ends at 8 or at 16 chunks");
  if (D <= 512) f(chunks<2>{});
  else if (D <= 768) f(chunks<3>{});
  else if (D <= 1024) f(chunks<4>{});
  else if (D <= 2048) f(chunks<8>{});
  else if constexpr (MAXCH > 8) f(chunks<MAXCH>{});
}
