// LoRA adapter kernels: the two memory-bound launches an adapted linear adds around the existing GEMMs.
//
//   vmc_lora_down_concat   out = [ x | round16(scale . x A16^T) | 0 ]: the rank-r projection of every row, written as the 64-column
//                          tail of the concat buffer the existing GEMM then reads as one more K tile.  The 16-row fragments of x that
//                          feed the MFMAs are the registers that are stored into out, so x is read once.
//   vmc_lora_wgrad_tn      out [r, C] (or [C, r]) = t^T x over the tokens: the adapter gradients.  Token slices -> fp32 slabs ->
//                          a sum in slice order (the scheme of gemm_tn.hip; no atomics, the same bits every call).
//
// Plans and argument checks: lora_route.h.
#include "common.h"
#include "lora_route.h"

// =============================================================================================================================
// down projection + concat
// =============================================================================================================================
// MFMA 16x16x32 as (A = adapter rows, B = x rows): lane (rr = lane & 15, g = lane >> 4) holds A16[16 nt + rr][k + 8 g ..+8] (from
// LDS) and x[m0 + rr][k + 8 g ..+8] (one 16-byte global load: a row of the fragment is 64 contiguous bytes), and receives
// D[j = 16 nt + 4 g + i][m = m0 + rr], i = 0..3: four consecutive tail columns of one row -> one 8-byte store.
template <typename T, int NT, int RT>
__global__ __launch_bounds__(256) void lora_down_kernel(const uint16_t* x, int ldx, const uint16_t* __restrict__ a16, int lda, uint16_t* out,
                                                        int ldo, int M, int K, int r, int col0, float scale, int copy_x, int kc) {
  extern __shared__ __attribute__((aligned(16))) char lora_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rr = lane & 15, g = lane >> 4;
  const int lds_ld = kc + 8;                                   // elements: 16-byte rows, 4 banks apart
  const long long row_base = (long long)blockIdx.x * (LORA_DOWN_ROWS * RT) + wave * 16 + rr;

  f32x4 acc[RT][NT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[t][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kb = 0; kb < K; kb += kc) {
    const int klen = min(kc, K - kb), chunks = klen >> 3;
    __syncthreads();                                           // the previous chunk has been read by every wave
    for (int idx = tid; idx < 16 * NT * chunks; idx += 256) {
      const int j = idx / chunks, ch = idx - j * chunks;
      uint4 v = make_uint4(0, 0, 0, 0);                        // rows r .. 16 NT of the adapter are zeros
      if (j < r) v = *(const uint4*)(a16 + (size_t)j * lda + kb + ch * 8);
      *(uint4*)(lora_smem + ((size_t)j * lds_ld + ch * 8) * 2) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const long long m = row_base + t * LORA_DOWN_ROWS;
      const bool live = m < M;
      const uint16_t* xp = x + (size_t)(live ? m : M - 1) * ldx + kb + 8 * g;      // rows past M: a valid row, never stored
      uint16_t* op = out + (size_t)(live ? m : 0) * ldo + kb + 8 * g;
      const bool copy = copy_x && live;
      for (int kk = 0; kk < klen; kk += 64) {                  // K % 64 == 0: two fragments (2 x 64 bytes of a row) per trip
        const uint4 xv0 = *(const uint4*)(xp + kk), xv1 = *(const uint4*)(xp + kk + 32);
        if (copy) {
          *(uint4*)(op + kk) = xv0;
          *(uint4*)(op + kk + 32) = xv1;
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const char* ap = lora_smem + ((size_t)(16 * n + rr) * lds_ld + kk + 8 * g) * 2;
          acc[t][n] = T::mfma16(*(const uint4*)ap, xv0, acc[t][n]);
          acc[t][n] = T::mfma16(*(const uint4*)(ap + 64), xv1, acc[t][n]);
        }
      }
    }
  }
  // the 64 tail columns: scale . acc rounded once to 16 bits for j < r, zeros behind (also where a padded adapter row met a
  // non-finite x: 0 . inf is not what the tail holds)
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const long long m = row_base + t * LORA_DOWN_ROWS;
    if (m >= M) continue;
    uint16_t* op = out + (size_t)m * ldo + col0 + 4 * g;
#pragma unroll
    for (int n = 0; n < LORA_TAIL / 16; ++n) {
      uint2 v = make_uint2(0, 0);
      if (n < NT) {
        if (16 * n + 4 * g < r) {
          const f32x4 a = acc[t][n < NT ? n : 0];
          v = make_uint2(T::pack(scale * a[0], scale * a[1]), T::pack(scale * a[2], scale * a[3]));
        }
      }
      *(uint2*)(op + 16 * n) = v;
    }
  }
}

template <typename T, int NT>
static int lora_down_launch_rt(const LoraDownPlan& p, const uint16_t* x, int ldx, const uint16_t* a16, int lda, uint16_t* out, int ldo, int M,
                               int K, int r, int col0, float scale, int copy_x, hipStream_t s) {
  if (p.rt == 2)
    lora_down_kernel<T, NT, 2><<<p.grid, 256, p.lds, s>>>(x, ldx, a16, lda, out, ldo, M, K, r, col0, scale, copy_x, p.kc);
  else
    lora_down_kernel<T, NT, 1><<<p.grid, 256, p.lds, s>>>(x, ldx, a16, lda, out, ldo, M, K, r, col0, scale, copy_x, p.kc);
  return (int)hipGetLastError();
}

extern "C" int vmc_lora_down_concat(const void* x, int ldx, const void* a16, int lda, void* out, int ldo, int M, int K, int r, int col0,
                                    float scale, int copy_x, int dtype16, void* stream) {
  const int rc = lora_check_down((uintptr_t)x, (uintptr_t)a16, (uintptr_t)out, ldx, lda, ldo, M, K, r, col0);
  if (rc) return rc;
  const LoraDownPlan p = lora_route_down(M, K, r);
  if (p.rc) return p.rc;
  return dispatch16(dtype16, [&](auto tag) {
    using T = decltype(tag);
    const uint16_t *xp = (const uint16_t*)x, *ap = (const uint16_t*)a16;
    uint16_t* o = (uint16_t*)out;
    hipStream_t s = (hipStream_t)stream;
    switch (p.nt) {
      case 1: return lora_down_launch_rt<T, 1>(p, xp, ldx, ap, lda, o, ldo, M, K, r, col0, scale, copy_x, s);
      case 2: return lora_down_launch_rt<T, 2>(p, xp, ldx, ap, lda, o, ldo, M, K, r, col0, scale, copy_x, s);
      case 3: return lora_down_launch_rt<T, 3>(p, xp, ldx, ap, lda, o, ldo, M, K, r, col0, scale, copy_x, s);
      default: return lora_down_launch_rt<T, 4>(p, xp, ldx, ap, lda, o, ldo, M, K, r, col0, scale, copy_x, s);
    }
  });
}

// =============================================================================================================================
// adapter gradients: out = t^T x over the tokens
// =============================================================================================================================
// A stage is 64 tokens of x (128 columns, LDS rows of 288 bytes) and of t (64 columns, rows of 160 bytes): consecutive rows start
// 8 banks apart, and the eight token rows that the two 16-lane groups of a half wave read together are rows 8 i .. 8 i + 7, so a
// ds_read_b64_tr_b16 touches every bank once.  The read hands lane rr the four tokens of column rr out of the 4 x 16 block its
// 16-lane group addresses (gemm_tn_body.h is the model); which tokens meet in an MFMA k slot is free, as long as both operands
// agree: k slot (g, e, i) is token 32 ks + 16 (g >> 1) + 8 e + 4 (g & 1) + i.
constexpr int LW_XLD = LORA_WG_COLS * 2 + 32, LW_TLD = LORA_TAIL * 2 + 32;

__device__ __forceinline__ uint2 lw_read_tr(const char* p) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  const v4s v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VMC_LDS v4s*)(uintptr_t)(const VMC_LDS char*)p);
  return __builtin_bit_cast(uint2, v);
}

template <typename T, int NT, bool TR>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const uint16_t* __restrict__ t, int ldt, const uint16_t* __restrict__ x, int ldx,
                                                         float* __restrict__ dst, int M, int r, int C, int tokens_per_slice) {
  __shared__ __attribute__((aligned(16))) char sx[LORA_WG_TOKENS * LW_XLD];
  __shared__ __attribute__((aligned(16))) char st[LORA_WG_TOKENS * LW_TLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rr = lane & 15, g = lane >> 4, q = rr >> 2, p = rr & 3;
  const int c0 = blockIdx.x * LORA_WG_COLS;
  const int m0 = blockIdx.y * tokens_per_slice, m1 = min(M, m0 + tokens_per_slice);
  float* outp = dst + (size_t)blockIdx.y * r * C;

  // staging: x 64 rows x 16 chunks of 16 bytes (four per thread), t 64 rows x 8 chunks (two per thread).  Chunks past the matrix
  // edge (columns >= C or >= r, token rows >= m1) are zeros and are not loaded: what lies beyond an operand is never read
  uint4 xr[4], tr[2];
  auto load = [&](int mb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = i * 256 + tid, row = id >> 4, c = c0 + (id & 15) * 8, m = mb + row;
      xr[i] = make_uint4(0, 0, 0, 0);
      if (m < m1 && c < C) xr[i] = *(const uint4*)(x + (size_t)m * ldx + c);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int id = i * 256 + tid, row = id >> 3, j = (id & 7) * 8, m = mb + row;
      tr[i] = make_uint4(0, 0, 0, 0);
      if (m < m1 && j < r) tr[i] = *(const uint4*)(t + (size_t)m * ldt + j);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = i * 256 + tid;
      *(uint4*)(sx + (id >> 4) * LW_XLD + (id & 15) * 16) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int id = i * 256 + tid;
      *(uint4*)(st + (id >> 3) * LW_TLD + (id & 7) * 16) = tr[i];
    }
  };

  f32x4 acc[2][NT];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[a][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int row_lane = 16 * (g >> 1) + 4 * (g & 1) + q;       // + 32 ks + 8 e
  load(m0);
  for (int mb = m0; mb < m1; mb += LORA_WG_TOKENS) {
    __syncthreads();                                           // the previous stage has been read
    stash();
    __syncthreads();
    if (mb + LORA_WG_TOKENS < m1) load(mb + LORA_WG_TOKENS);   // in flight under the MFMAs of this stage
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 xf[2], tf[NT];
      const int row = 32 * ks + row_lane;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const char* b = sx + row * LW_XLD + (wave * 32 + a * 16 + 4 * p) * 2;
        const uint2 lo = lw_read_tr(b), hi = lw_read_tr(b + 8 * LW_XLD);
        xf[a] = make_uint4(lo.x, lo.y, hi.x, hi.y);
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const char* b = st + row * LW_TLD + (n * 16 + 4 * p) * 2;
        const uint2 lo = lw_read_tr(b), hi = lw_read_tr(b + 8 * LW_TLD);
        tf[n] = make_uint4(lo.x, lo.y, hi.x, hi.y);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = TR ? T::mfma16(tf[n], xf[a], acc[a][n]) : T::mfma16(xf[a], tf[n], acc[a][n]);
    }
  }
  // (x, t): the lane holds out[j = 16 n + rr][c = cbase + 4 g ..+4]; (t, x): out^T[c = cbase + rr][j = 16 n + 4 g ..+4].  Either way
  // four consecutive floats of a row: one 16-byte store (r % 8 == 0, C % 8 == 0: a started group of four never crosses the edge)
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int cb = c0 + wave * 32 + a * 16;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const float4 v = make_float4(acc[a][n][0], acc[a][n][1], acc[a][n][2], acc[a][n][3]);
      if (TR) {
        const int c = cb + rr, j = 16 * n + 4 * g;
        if (c < C && j < r) *(float4*)(outp + (size_t)c * r + j) = v;
      } else {
        const int c = cb + 4 * g, j = 16 * n + rr;
        if (c < C && j < r) *(float4*)(outp + (size_t)j * C + c) = v;
      }
    }
  }
}

// out[i] = slab 0 [i] + slab 1 [i] + ... in slice order (n4 groups of four floats)
__global__ __launch_bounds__(256) void lora_slab_sum_kernel(const float4* __restrict__ slabs, float4* __restrict__ out, size_t n4, int slices) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 s = slabs[i];
    for (int k0 = 1; k0 < slices; k0 += 8) {       // eight loads in flight, added in slice order
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = k0 + u < slices ? slabs[(size_t)(k0 + u) * n4 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < slices) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    out[i] = s;
  }
}

template <typename T, int NT>
static int lora_wgrad_launch(const LoraWgradPlan& p, const uint16_t* t, int ldt, const uint16_t* x, int ldx, float* dst, int M, int r, int C,
                             int transpose_out, hipStream_t s) {
  const dim3 grid(p.c_tiles, p.slices);
  if (transpose_out) lora_wgrad_kernel<T, NT, true><<<grid, 256, 0, s>>>(t, ldt, x, ldx, dst, M, r, C, p.tokens_per_slice);
  else lora_wgrad_kernel<T, NT, false><<<grid, 256, 0, s>>>(t, ldt, x, ldx, dst, M, r, C, p.tokens_per_slice);
  return (int)hipGetLastError();
}

extern "C" size_t vmc_lora_wgrad_tn_workspace_bytes(int M, int r, int C) {
  const LoraWgradPlan p = lora_route_wgrad(M, r, C);
  return p.rc ? 0 : p.workspace_bytes;
}

extern "C" int vmc_lora_wgrad_tn(const void* t, int ldt, const void* x, int ldx, float* out, int M, int r, int C, int transpose_out,
                                 void* workspace, size_t workspace_bytes, int dtype16, void* stream) {
  const int rc = lora_check_wgrad((uintptr_t)t, (uintptr_t)x, (uintptr_t)out, ldt, ldx, M, r, C, (uintptr_t)workspace, workspace_bytes);
  if (rc) return rc;
  const LoraWgradPlan p = lora_route_wgrad(M, r, C);
  hipStream_t s = (hipStream_t)stream;
  float* dst = p.slices > 1 ? (float*)workspace : out;
  const int lrc = dispatch16(dtype16, [&](auto tag) {
    using T = decltype(tag);
    const uint16_t *tp = (const uint16_t*)t, *xp = (const uint16_t*)x;
    switch (p.nt) {
      case 1: return lora_wgrad_launch<T, 1>(p, tp, ldt, xp, ldx, dst, M, r, C, transpose_out, s);
      case 2: return lora_wgrad_launch<T, 2>(p, tp, ldt, xp, ldx, dst, M, r, C, transpose_out, s);
      case 3: return lora_wgrad_launch<T, 3>(p, tp, ldt, xp, ldx, dst, M, r, C, transpose_out, s);
      default: return lora_wgrad_launch<T, 4>(p, tp, ldt, xp, ldx, dst, M, r, C, transpose_out, s);
    }
  });
  if (lrc || p.slices == 1) return lrc;
  const size_t n4 = (size_t)r * C / 4;
  lora_slab_sum_kernel<<<grid_for(n4, 256), 256, 0, s>>>((const float4*)workspace, (float4*)out, n4, p.slices);
  return (int)hipGetLastError();
}
