// Contrastive (symmetric InfoNCE) distillation: the memory-bound kernels around the two MFMA GEMMs (gfx950, fp32 math).
//
//   prep      s, t  ->  u16 = round16(s / max(|s|, eps)), v16 likewise, v16^T, inv_s            (one wave per row + a tile transpose)
//   GEMM      z = (1 / tau) u16 v16^T                                                             (vmc_linear, not here)
//   softmax   z     ->  masked row / column log-sum-exp, loss, top-1 count, dz16                  (four launches, see below)
//   GEMM      du = dz16 v16 / (2 M tau)                                                           (vmc_linear, not here)
//   norm_bwd  du, s ->  ds through the normalisation, the clamp branch included                   (one wave per row)
//
// Pair (i, j) is valid when clip(j) != clip(i) or j == i, clip(i) = i / rows_per_clip (rows_per_clip == 0: every pair).  Every
// reduction runs in a fixed order -- lanes, then a butterfly whose lane-0 result is taken, strips in ascending order -- and nothing
// is added with atomics: the same input gives the same bits.
//
// The diagonal is kept out of every running sum and added last: with rest = sum over the valid j != i of exp(z_ij - m),
//   1 - p_ii = rest / (rest + exp(z_ii - m))
// has the relative accuracy of a sum, so that neither the loss term -log p_ii nor dz_ii = p_row_ii + p_col_ii - 2 is formed as a
// difference of numbers near 1 and 2.
#include <math.h>

#include "common.h"

static constexpr int CON_MAX_ROWS = 16384;
static constexpr int CON_STRIP = 32;          // rows of z per workgroup of the statistics pass = rows per column partial
static constexpr float CON_EPS = 1e-5f;       // the cosine mode's clamp (losses.py:27)

static inline int con_pad(int M) { return (M + 63) / 64 * 64; }
static inline int con_strips(int M) { return (M + CON_STRIP - 1) / CON_STRIP; }
static inline size_t con_align(size_t bytes) { return (bytes + 255) / 256 * 256; }
static inline bool con_rows_ok(int M) { return M >= 1 && M <= CON_MAX_ROWS; }
static inline bool con_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- running (max, sum of exp) pairs -----------------------------------------------------------------------------------------
// (m, s) stands for s * exp(m); the empty pair is (-inf, 0).
__device__ inline void ms_add(float& m, float& s, float v) {
  const float d = v - m;                       // +inf on the first element
  const float e = expf(-fabsf(d));
  if (d > 0.f) { s = s * e + 1.0f; m = v; } else { s += e; }
}
__device__ inline void ms_merge(float& m, float& s, float m2, float s2) {
#pragma clang fp contract(off)                 // both lanes of a butterfly pair must round alike
  const float mn = fmaxf(m, m2);
  const float a = (m == mn) ? 1.0f : expf(m - mn);       // the comparison keeps (-inf) - (-inf) out of expf
  const float b = (m2 == mn) ? 1.0f : expf(m2 - mn);
  s = s * a + s2 * b;
  m = mn;
}
// (m, s) over the valid entries beside the diagonal, zd the diagonal: log-sum-exp, -log p_diag and 1 - p_diag.
__device__ inline void con_finish(float m, float s, float zd, float& lse, float& term, float& q) {
  const float mm = fmaxf(m, zd);
  const float rest = s * ((m == mm) ? 1.0f : expf(m - mm));
  const float sum = rest + expf(zd - mm);
  const float ls = logf(sum);
  q = rest / sum;
  lse = mm + ls;
  term = q < 0.5f ? -log1pf(-q) : (mm - zd) + ls;
}

// ---- prep -------------------------------------------------------------------------------------------------------------------
__device__ inline float con_row_sumsq(const float* __restrict__ r, int E, int lane) {
  float a = 0.f;
  for (int i = lane * 2; i < E; i += 128) a += r[i] * r[i] + r[i + 1] * r[i + 1];
  return wave_sum(a);
}

// One wave per row of the padded [Mp, E] outputs; E % 64 == 0, so every lane owns whole pairs.
template <typename T>
__global__ void __launch_bounds__(256) con_prep_kernel(const float* __restrict__ s, const float* __restrict__ t, uint32_t* __restrict__ u16,
                                                       uint32_t* __restrict__ v16, float* __restrict__ inv_s, int M, int Mp, int E,
                                                       int rows_per_clip, size_t clip_stride) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Mp) return;
  uint32_t* ur = u16 + (size_t)row * (E / 2);
  uint32_t* vr = v16 + (size_t)row * (E / 2);
  if (row >= M) {                              // pad rows: the second GEMM contracts over them
    for (int i = lane; i < E / 2; i += 64) { ur[i] = 0u; vr[i] = 0u; }
    return;
  }
  const float* sr = s + (size_t)row * E;
  const float* tr = t + (size_t)(row / rows_per_clip) * clip_stride + (size_t)(row % rows_per_clip) * E;
  const float is = 1.0f / fmaxf(sqrtf(con_row_sumsq(sr, E, lane)), CON_EPS);
  const float it = 1.0f / fmaxf(sqrtf(con_row_sumsq(tr, E, lane)), CON_EPS);
  if (lane == 0) inv_s[row] = is;
  for (int i = lane * 2; i < E; i += 128) {
    ur[i >> 1] = pack2<T>(sr[i] * is, sr[i + 1] * is);
    vr[i >> 1] = pack2<T>(tr[i] * it, tr[i + 1] * it);
  }
}

extern "C" int vmc_contrastive_prep(const float* student, const float* teacher, void* u16, void* v16, void* vt16, float* inv_s, int M,
                                    int E, int rows_per_clip, size_t teacher_clip_stride, int dtype16, void* stream) {
  if (!student || !teacher || !u16 || !v16 || !vt16 || !inv_s || rows_per_clip <= 0) return VMC_E_ARG;
  if (!con_rows_ok(M) || E < 64 || E % 64 != 0) return VMC_E_SHAPE;
  if (!con_aligned(u16, 16) || !con_aligned(v16, 16) || !con_aligned(vt16, 16)) return VMC_E_ALIGN;
  const int Mp = con_pad(M);
  const hipStream_t s = (hipStream_t)stream;
  const int rc = dispatch16(dtype16, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(con_prep_kernel<T>, dim3(Mp / 4), dim3(256), 0, s, student, teacher, (uint32_t*)u16, (uint32_t*)v16, inv_s, M, Mp, E,
                       rows_per_clip, teacher_clip_stride);
    return (int)hipGetLastError();
  });
  if (rc) return rc;
  return vmc_transpose16(v16, vt16, Mp, E, E, Mp, stream);       // a copy of the rounded bits: pad rows become pad columns
}

// ---- softmax ----------------------------------------------------------------------------------------------------------------
// Partials (floats): pm, ps [strips, M] | row_term, col_term, q_row, q_col [M] | hit [M] (int32).
struct ConPartials {
  float *pm, *ps, *row_term, *col_term, *q_row, *q_col;
  int* hit;
};
static inline ConPartials con_partials(void* base, int M) {
  float* f = (float*)base;
  const size_t n = (size_t)con_strips(M) * M;
  return {f, f + n, f + 2 * n, f + 2 * n + M, f + 2 * n + 2 * (size_t)M, f + 2 * n + 3 * (size_t)M, (int*)(f + 2 * n + 4 * (size_t)M)};
}
extern "C" size_t vmc_contrastive_partials_bytes(int M) {
  if (!con_rows_ok(M)) return 0;
  return (2 * (size_t)con_strips(M) * M + 5 * (size_t)M) * sizeof(float);
}

// A strip of CON_STRIP rows per workgroup.  First one wave per row: the row's statistics.  Then one thread per column: the strip's
// share of the column's (max, sum), read along the rows (consecutive lanes, consecutive columns).
__global__ void __launch_bounds__(256) con_stats_kernel(const float* __restrict__ z, int M, size_t ldz, int T, float* __restrict__ lse_row,
                                                        ConPartials p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * CON_STRIP;
  const int r1 = min(r0 + CON_STRIP, M);
  for (int i = r0 + wave; i < r1; i += 4) {
    const float* zr = z + (size_t)i * ldz;
    const int c0 = T > 0 ? (i / T) * T : 0, c1 = T > 0 ? c0 + T : 0;      // the row's own clip
    float m = -INFINITY, s = 0.f;
    for (int j = lane; j < M; j += 64) {
      if ((j >= c0 && j < c1) || j == i) continue;
      ms_add(m, s, zr[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ms_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    m = __shfl(m, 0, 64);
    s = __shfl(s, 0, 64);
    if (lane == 0) {
      const float zd = zr[i];
      float lse, term, q;
      con_finish(m, s, zd, lse, term, q);
      lse_row[i] = lse;
      p.row_term[i] = term;
      p.q_row[i] = q;
      p.hit[i] = zd >= m ? 1 : 0;             // no valid entry beside the diagonal: m = -inf, a hit
    }
  }
  for (int j = threadIdx.x; j < M; j += 256) {
    const int c0 = T > 0 ? (j / T) * T : 0, c1 = T > 0 ? c0 + T : 0;
    float m = -INFINITY, s = 0.f;
    for (int r = r0; r < r1; ++r) {
      if ((r >= c0 && r < c1) || r == j) continue;
      ms_add(m, s, z[(size_t)r * ldz + j]);
    }
    p.pm[(size_t)blockIdx.x * M + j] = m;
    p.ps[(size_t)blockIdx.x * M + j] = s;
  }
}

// One thread per column: the strips' partials in ascending order, then the diagonal.
__global__ void __launch_bounds__(256) con_columns_kernel(const float* __restrict__ z, int M, size_t ldz, int strips,
                                                          float* __restrict__ lse_col, ConPartials p) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  float m = -INFINITY, s = 0.f;
  for (int k = 0; k < strips; ++k) ms_merge(m, s, p.pm[(size_t)k * M + j], p.ps[(size_t)k * M + j]);
  float lse, term, q;
  con_finish(m, s, z[(size_t)j * ldz + j], lse, term, q);
  lse_col[j] = lse;
  p.col_term[j] = term;
  p.q_col[j] = q;
}

// loss = sum_i (-log p_row_ii - log p_col_ii) / (2 M) and the number of hits, one workgroup, fixed order.
__global__ void __launch_bounds__(256) con_reduce_kernel(ConPartials p, int M, float* __restrict__ loss, int* __restrict__ top1) {
  __shared__ float sm[4];
  __shared__ int sn[4];
  float a = 0.f;
  int n = 0;
  for (int i = threadIdx.x; i < M; i += 256) {
    a += p.row_term[i] + p.col_term[i];
    n += p.hit[i];
  }
  a = wave_sum(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = a; sn[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = ((sm[0] + sm[1]) + (sm[2] + sm[3])) * (0.5f / (float)M);
    top1[0] = (sn[0] + sn[1]) + (sn[2] + sn[3]);
  }
}

// dz16[i, j] = round16(p_row_ij + p_col_ij - 2 delta_ij) on valid pairs, 0 elsewhere and in the pad columns.  One wave per row, two
// columns per lane: 4-byte stores.
template <typename T>
__global__ void __launch_bounds__(256) con_grad_kernel(const float* __restrict__ z, int M, int Mp, size_t ldz, int Tc,
                                                       const float* __restrict__ lse_row, const float* __restrict__ lse_col, ConPartials p,
                                                       uint32_t* __restrict__ dz16) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  const float* zr = z + (size_t)i * ldz;
  uint32_t* out = dz16 + (size_t)i * (Mp / 2);
  const int c0 = Tc > 0 ? (i / Tc) * Tc : 0, c1 = Tc > 0 ? c0 + Tc : 0;
  const float lr = lse_row[i];
  const float diag = 0.0f - (p.q_row[i] + p.q_col[i]);
  auto elem = [&](int j) -> float {
    if (j >= M) return 0.0f;                   // pad column: z is not read there
    if (j == i) return diag;
    if (j >= c0 && j < c1) return 0.0f;
    const float v = zr[j];
    return expf(v - lr) + expf(v - lse_col[j]);
  };
  for (int j = lane * 2; j < Mp; j += 128) out[j >> 1] = pack2<T>(elem(j), elem(j + 1));
}

extern "C" int vmc_contrastive_softmax(const float* z, int M, int ldz, int rows_per_clip, float* lse_row, float* lse_col, float* loss,
                                       int* top1, void* dz16, int dtype16, void* partials, size_t partials_bytes, void* stream) {
  if (!z || !lse_row || !lse_col || !loss || !top1 || !partials || rows_per_clip < 0) return VMC_E_ARG;
  if (!con_rows_ok(M)) return VMC_E_SHAPE;
  if (ldz < M || partials_bytes < vmc_contrastive_partials_bytes(M)) return VMC_E_ARG;
  if (dtype16 != VMC_BF16 && dtype16 != VMC_F16) return VMC_E_DTYPE;
  if (!con_aligned(partials, 4) || !con_aligned(z, 4) || (dz16 && !con_aligned(dz16, 4))) return VMC_E_ALIGN;
  const hipStream_t s = (hipStream_t)stream;
  const ConPartials p = con_partials(partials, M);
  const int strips = con_strips(M), Mp = con_pad(M);
  hipLaunchKernelGGL(con_stats_kernel, dim3(strips), dim3(256), 0, s, z, M, (size_t)ldz, rows_per_clip, lse_row, p);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(con_columns_kernel, dim3((M + 255) / 256), dim3(256), 0, s, z, M, (size_t)ldz, strips, lse_col, p);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(con_reduce_kernel, dim3(1), dim3(256), 0, s, p, M, loss, top1);
  VMC_CHECK_LAUNCH();
  if (!dz16) return 0;
  return dispatch16(dtype16, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(con_grad_kernel<T>, dim3((M + 3) / 4), dim3(256), 0, s, z, M, Mp, (size_t)ldz, rows_per_clip, (const float*)lse_row,
                       (const float*)lse_col, p, (uint32_t*)dz16);
    return (int)hipGetLastError();
  });
}

// ---- norm_bwd ---------------------------------------------------------------------------------------------------------------
// u = s inv_s:  ds = inv_s (du - u (u . du)) where |s| > eps;  ds = du / eps where the clamp holds the norm (torch's gradient of
// clamp: nothing flows through the norm).  ds may be du itself: a lane rewrites only what it has read, after the row's dot product.
__global__ void __launch_bounds__(256) con_norm_bwd_kernel(const float* du, const float* __restrict__ s, const float* __restrict__ inv_s,
                                                           float* ds, int M, int E) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* sr = s + (size_t)row * E;
  const float* gr = du + (size_t)row * E;
  float* out = ds + (size_t)row * E;
  const bool free_norm = sqrtf(con_row_sumsq(sr, E, lane)) > CON_EPS;      // the sum prep formed, bit for bit
  if (!free_norm) {
    for (int i = lane; i < E; i += 64) out[i] = gr[i] / CON_EPS;
    return;
  }
  float dot = 0.f;
  for (int i = lane; i < E; i += 64) dot += sr[i] * gr[i];
  const float is = inv_s[row];
  const float k = wave_sum(dot) * is * is;                                 // (u . du) inv_s
  for (int i = lane; i < E; i += 64) out[i] = is * (gr[i] - sr[i] * k);
}

extern "C" int vmc_contrastive_norm_bwd(const float* du, const float* student, const float* inv_s, float* dstudent, int M, int E,
                                        void* stream) {
  if (!du || !student || !inv_s || !dstudent) return VMC_E_ARG;
  if (!con_rows_ok(M) || E < 64 || E % 64 != 0) return VMC_E_SHAPE;
  hipLaunchKernelGGL(con_norm_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, du, student, inv_s, dstudent, M, E);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- workspace --------------------------------------------------------------------------------------------------------------
// u16 | v16 | v16^T | z | dz16 | lse_row | lse_col | partials, every part on a 256-byte boundary.
extern "C" int vmc_contrastive_workspace_layout(int M, int E, size_t* offsets) {
  if (!offsets) return VMC_E_ARG;
  if (!con_rows_ok(M) || E < 64 || E % 64 != 0) return VMC_E_SHAPE;
  const size_t Mp = (size_t)con_pad(M);
  const size_t part[8] = {Mp * E * 2, Mp * E * 2, Mp * E * 2, (size_t)M * Mp * 4, (size_t)M * Mp * 2, (size_t)M * 4, (size_t)M * 4,
                          vmc_contrastive_partials_bytes(M)};
  size_t at = 0;
  for (int i = 0; i < 8; ++i) {
    offsets[i] = at;
    at += con_align(part[i]);
  }
  offsets[8] = at;
  return 0;
}
extern "C" size_t vmc_contrastive_workspace_bytes(int M, int E) {
  size_t off[9];
  return vmc_contrastive_workspace_layout(M, E, off) == 0 ? off[8] : 0;
}
