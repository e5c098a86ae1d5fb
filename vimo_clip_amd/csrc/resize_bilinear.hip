// Bilinear resize of u8 frames to f32 in [0,1] or to the u8 pixels PIL makes of them (gfx950): the arithmetic of the reference's
// dataset_frame_diff_mn.py `_resize_frames` (frames.float() / 255 -> F.interpolate(mode="bilinear", align_corners=False)) and of
// the `to_pil_image` that follows it in the student (pic.mul(255).byte()), bit for bit.
//
// The recipes (DESIGN.md "Bilinear resize"): everything is float32 and every operation is rounded once, in aten's order.
//     scale = (float)in / (float)out
//     src   = fma(scale, d + 0.5, -0.5), clamped at 0;  i0 = min((int)src, in-1);  i1 = min(i0+1, in-1)
//     l1    = clamp(src - i0, 0, 1);  l0 = 1 - l1
//     p(v)  = v / 255                                   correctly rounded: a 256-entry table the COMPILER divides (IEEE, on the host)
//   separable (aten's generic kernel):
//     row(y)= fma(lx0, p[y][x0], lx1 * p[y][x1])        the product lx1 * p is rounded first
//     out   = fma(ly0, row(y0), ly1 * row(y1))
//   four weights (aten's channels-last kernel, which it also runs on small outputs and in one-thread processes):
//     wYX   = lyY * lxX                                 four rounded products
//     out   = fma(w11, p11, fma(w10, p10, fma(w00, p00, w01 * p01)))
//     q     = (u8) trunc(out * 255)
// aten picks between the two by output size and thread count, so the caller names the recipe or asks for aten's own choice in a
// multi-threaded process (four weights when OH + OW <= VMC_RESIZE_ATEN_SMALL).  hipcc contracts a * b + c on its own, which would give
// one of the variants that match NEITHER; every operation below is therefore an explicit round-to-nearest intrinsic.
//
// Bandwidth bound: 1 B (mode 1) or 4 B (mode 0) written per output sample, the source read once from HBM (the 2 x 2 taps of
// neighbouring outputs share cache lines).  A block owns RB_ROWS output rows x RB_TX output columns of one plane:
//   * the x tables (tap columns and weights) are computed once per block, one thread per output column, into LDS, and p(v) is copied
//     into LDS beside them; a thread then keeps the tables of its RB_PX = 4 consecutive columns in registers for all its rows;
//   * a wave owns one output row at a time, so the y table is wave-uniform;
//   * one 16-byte (f32) or 4-byte (u8) store per thread where four whole outputs sit at an aligned address, chosen per thread from the
//     address itself; a ragged row end, an OW that is no multiple of 4 and an unaligned `dst` take scalar stores of the same values.
#include "common.h"

#define RB_TX 256            // output columns per block = threads per block (one column each while the x tables are built)
#define RB_PX 4              // consecutive output columns per thread
#define RB_ROWS 8            // output rows per block (two per wave)

struct RbUnit {
  float v[256];
  constexpr RbUnit() : v() {
    for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
  }
};
__device__ const RbUnit rb_unit = RbUnit();

// Source taps and weights of output index d along one axis (aten's area_pixel_compute_source_index + guard_index_and_lambda).
__device__ __forceinline__ void rb_axis(int d, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  float src = __fmaf_rn(scale, __fadd_rn((float)d, 0.5f), -0.5f);
  if (src < 0.0f) src = 0.0f;
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.0f), 1.0f);
  l0 = __fsub_rn(1.0f, l1);
}

__device__ __forceinline__ uint32_t rb_quant(float x) { return (uint32_t)((int)truncf(__fmul_rn(x, 255.0f)) & 255); }

template <int MODE, int RECIPE>
__global__ void __launch_bounds__(RB_TX) resize_bilinear_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, int C, int H, int W,
                                                                int OH, int OW, long long s_f, long long s_c, long long s_y, long long s_x,
                                                                float scale_y, float scale_x, int xtiles, int rtiles) {
  __shared__ float s_p[256];
  __shared__ int s_x0[RB_TX], s_x1[RB_TX];
  __shared__ float s_l0[RB_TX], s_l1[RB_TX];
  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int xt = (int)(b % (unsigned)xtiles);
  b /= (unsigned)xtiles;
  const int rt = (int)(b % (unsigned)rtiles);
  b /= (unsigned)rtiles;                       // b = f * C + c: the output plane
  const int c = (int)(b % (unsigned)C);
  const long long f = (long long)(b / (unsigned)C);

  s_p[tid] = rb_unit.v[tid];
  {
    const int ox = xt * RB_TX + tid;
    int i0 = 0, i1 = 0;
    float l0 = 0.0f, l1 = 0.0f;                // columns past OW: tap column 0 (in bounds), never stored
    if (ox < OW) rb_axis(ox, scale_x, W, i0, i1, l0, l1);
    s_x0[tid] = i0;
    s_x1[tid] = i1;
    s_l0[tid] = l0;
    s_l1[tid] = l1;
  }
  __syncthreads();

  const int g = tid & 63, wave = tid >> 6;
  const int gx = xt * RB_TX + g * RB_PX;
  if (gx >= OW) return;
  const int n = OW - gx < RB_PX ? OW - gx : RB_PX;
  long long a0[RB_PX], a1[RB_PX];
  float lx0[RB_PX], lx1[RB_PX];
#pragma unroll
  for (int j = 0; j < RB_PX; ++j) {
    a0[j] = (long long)s_x0[g * RB_PX + j] * s_x;
    a1[j] = (long long)s_x1[g * RB_PX + j] * s_x;
    lx0[j] = s_l0[g * RB_PX + j];
    lx1[j] = s_l1[g * RB_PX + j];
  }
  const uint8_t* plane = src + f * s_f + (long long)c * s_c;
  for (int k = wave; k < RB_ROWS; k += RB_TX / 64) {
    const int oy = rt * RB_ROWS + k;
    if (oy >= OH) break;
    int y0, y1;
    float ly0, ly1;
    rb_axis(oy, scale_y, H, y0, y1, ly0, ly1);
    const uint8_t* r0 = plane + (long long)y0 * s_y;
    const uint8_t* r1 = plane + (long long)y1 * s_y;
    float o[RB_PX];
#pragma unroll
    for (int j = 0; j < RB_PX; ++j) {
      const float p00 = s_p[r0[a0[j]]], p01 = s_p[r0[a1[j]]], p10 = s_p[r1[a0[j]]], p11 = s_p[r1[a1[j]]];
      if (RECIPE == VMC_RESIZE_SEPARABLE) {
        const float top = __fmaf_rn(lx0[j], p00, __fmul_rn(lx1[j], p01));
        const float bot = __fmaf_rn(lx0[j], p10, __fmul_rn(lx1[j], p11));
        o[j] = __fmaf_rn(ly0, top, __fmul_rn(ly1, bot));
      } else {
        const float w00 = __fmul_rn(ly0, lx0[j]), w01 = __fmul_rn(ly0, lx1[j]), w10 = __fmul_rn(ly1, lx0[j]), w11 = __fmul_rn(ly1, lx1[j]);
        o[j] = __fmaf_rn(w11, p11, __fmaf_rn(w10, p10, __fmaf_rn(w00, p00, __fmul_rn(w01, p01))));
      }
    }
    const size_t off = ((size_t)b * OH + oy) * OW + gx;
    if (MODE == 0) {
      float* q = (float*)dst + off;
      if (n == RB_PX && ((uintptr_t)q & 15) == 0) {
        *(f32x4*)q = (f32x4){o[0], o[1], o[2], o[3]};
      } else {
#pragma unroll
        for (int j = 0; j < RB_PX; ++j)
          if (j < n) q[j] = o[j];
      }
    } else {
      uint8_t* q = (uint8_t*)dst + off;
      if (n == RB_PX && ((uintptr_t)q & 3) == 0) {
        *(uint32_t*)q = rb_quant(o[0]) | (rb_quant(o[1]) << 8) | (rb_quant(o[2]) << 16) | (rb_quant(o[3]) << 24);
      } else {
#pragma unroll
        for (int j = 0; j < RB_PX; ++j)
          if (j < n) q[j] = (uint8_t)rb_quant(o[j]);
      }
    }
  }
}

extern "C" int vmc_resize_bilinear_u8(const uint8_t* src, void* dst, int F, int C, int H, int W, int OH, int OW, long long s_f,
                                      long long s_c, long long s_y, long long s_x, int out_mode, void* stream) {
  if (!src || !dst || F < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return VMC_E_ARG;
  if (C != 1 && C != 3) return VMC_E_ARG;
  if (out_mode < 0 || out_mode > (VMC_RESIZE_U8 | VMC_RESIZE_WEIGHTS4)) return VMC_E_ARG;
  int recipe = out_mode & (VMC_RESIZE_SEPARABLE | VMC_RESIZE_WEIGHTS4);
  if (recipe == (VMC_RESIZE_SEPARABLE | VMC_RESIZE_WEIGHTS4)) return VMC_E_ARG;
  if (recipe == 0) recipe = (long long)OH + OW <= VMC_RESIZE_ATEN_SMALL ? VMC_RESIZE_WEIGHTS4 : VMC_RESIZE_SEPARABLE;
  const bool u8 = (out_mode & VMC_RESIZE_U8) != 0;
  const int xtiles = (OW + RB_TX - 1) / RB_TX, rtiles = (OH + RB_ROWS - 1) / RB_ROWS;
  const unsigned long long blocks = (unsigned long long)xtiles * rtiles * (unsigned long long)F * C;
  if (blocks > 0x7FFFFFFFull) return VMC_E_SHAPE;
  const float scale_y = (float)H / (float)OH, scale_x = (float)W / (float)OW;
  hipStream_t s = (hipStream_t)stream;
#define RB_LAUNCH(MODE, RECIPE)                                                                                                   \
  hipLaunchKernelGGL((resize_bilinear_kernel<MODE, RECIPE>), dim3((unsigned)blocks), dim3(RB_TX), 0, s, src, dst, C, H, W, OH, OW, s_f, \
                     s_c, s_y, s_x, scale_y, scale_x, xtiles, rtiles)
  if (recipe == VMC_RESIZE_SEPARABLE) {
    if (u8) RB_LAUNCH(1, VMC_RESIZE_SEPARABLE); else RB_LAUNCH(0, VMC_RESIZE_SEPARABLE);
  } else {
    if (u8) RB_LAUNCH(1, VMC_RESIZE_WEIGHTS4); else RB_LAUNCH(0, VMC_RESIZE_WEIGHTS4);
  }
#undef RB_LAUNCH
  VMC_CHECK_LAUNCH();
  return 0;
}

// out[i] = (u8)(trunc(x[i] * 255) & 255): torchvision's to_pil_image on a float picture (pic.mul(255).byte()).  Four floats per thread
// as one 16-byte load and one 4-byte store where both pointers allow it; the last n % 4 elements, and everything when a pointer is
// unaligned, go one by one.
template <bool VEC>
__global__ void __launch_bounds__(256) unit_f32_to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = VEC ? n / 4 : 0;
  for (long long i = t; i < n4; i += stride) {
    const f32x4 v = ((const f32x4*)x)[i];
    ((uint32_t*)out)[i] = rb_quant(v[0]) | (rb_quant(v[1]) << 8) | (rb_quant(v[2]) << 16) | (rb_quant(v[3]) << 24);
  }
  for (long long i = n4 * 4 + t; i < n; i += stride) out[i] = (uint8_t)rb_quant(x[i]);
}

extern "C" int vmc_unit_f32_to_u8(const float* x, uint8_t* out, long long n, void* stream) {
  if (!x || !out || n < 1) return VMC_E_ARG;
  const bool vec = (((uintptr_t)x & 15) | ((uintptr_t)out & 3)) == 0;
  const int grid = grid_for((size_t)(vec ? (n + 3) / 4 : n), 256);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(unit_f32_to_u8_kernel<true>, dim3(grid), dim3(256), 0, s, x, out, n);
  else
    hipLaunchKernelGGL(unit_f32_to_u8_kernel<false>, dim3(grid), dim3(256), 0, s, x, out, n);
  VMC_CHECK_LAUNCH();
  return 0;
}
