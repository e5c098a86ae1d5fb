// K19 -- token concatenation at device-resident lengths (gfx950): the TFAM token-concatenation mode's
// torch.cat([rgb[:, :-1], motion], 1) (TFAM/models/AMO_CLIP.py:153-156) for a batch whose streams were zero-padded beyond their own
// lengths n_rgb / n_motion, with the real rows written as a PREFIX of the output:
//   x[b] = [ rgb[b, 0 .. n_rgb-2] | motion[b, 0 .. n_motion-1] | zeros up to T_out ],  the key mask laid out the same way,
//   pool_len = n_rgb - 1 + n_motion.
// The split position is a device value (it changes from one graph replay to the next), which is why torch.cat cannot build this.
//
// Pure data movement, ~1.5 MB at B = 8, T_out = 64, D = 768, read + written once: launch-latency bound, no LDS, no reuse.
//   grid = (ceil(T_out / CT_ROWS), B), 256 threads; a workgroup owns CT_ROWS = 4 consecutive output rows of one clip (128 workgroups
//   at the shape above, the same geometry as the store's gather, clip_store.hip).  The source of a row (rgb / motion / zero) is
//   uniform over the workgroup's threads; 16 bytes per lane where D % 4 == 0 and rgb, motion and x are 16-byte aligned (the host
//   decides), otherwise 4 bytes.  The workgroups with blockIdx.x == 0 also write their clip's mask row; thread 0 of workgroup (0, 0)
//   writes pool_len with a plain store.  Every element of x, mask and pool_len is written on every call.
//
// BOUNDS.  len_rgb / len_motion are device memory the host cannot validate.  Every thread clamps them the same way before any
// address is formed: nr into [1, T_rgb], nm into [1, T_motion], keep = min(nr - 1, T_out), nm = min(nm, T_out - keep),
// n = keep + nm in [1, T_out].  A source row index is then < keep <= T_rgb - 1 (rgb) or < nm <= T_motion (motion), a destination row
// < T_out.
#include "common.h"

#define CT_ROWS 4

struct CtArgs {
  const float* rgb;
  const float* motion;
  const uint8_t* mask_rgb;
  const uint8_t* mask_motion;
  float* x;
  uint8_t* mask;
  int* pool_len;
  const int* len_rgb;
  const int* len_motion;
  int B, T_rgb, T_motion, T_out, D;
  int vec;        // 16-byte path: D % 4 == 0, rgb, motion and x 16-byte aligned
};

__global__ void __launch_bounds__(256) concat_tokens_len_kernel(const CtArgs a) {
  const int b = blockIdx.y;
  const int T_out = a.T_out, D = a.D;
  int nr = a.len_rgb != nullptr ? *a.len_rgb : a.T_rgb;
  int nm = a.len_motion != nullptr ? *a.len_motion : a.T_motion;
  nr = nr < 1 ? 1 : (nr > a.T_rgb ? a.T_rgb : nr);
  nm = nm < 1 ? 1 : (nm > a.T_motion ? a.T_motion : nm);
  const int keep = nr - 1 < T_out ? nr - 1 : T_out;
  nm = nm < T_out - keep ? nm : T_out - keep;
  const int n = keep + nm;

  const int t0 = blockIdx.x * CT_ROWS;
  const int t1 = t0 + CT_ROWS < T_out ? t0 + CT_ROWS : T_out;
  for (int t = t0; t < t1; ++t) {
    const float* src = nullptr;                                         // nullptr: a zero row
    if (t < keep) {
      src = a.rgb + ((size_t)b * a.T_rgb + t) * D;
    } else if (t < n) {
      src = a.motion + ((size_t)b * a.T_motion + (t - keep)) * D;
    }
    float* dst = a.x + ((size_t)b * T_out + t) * D;
    if (a.vec) {
      const int D4 = D >> 2;
      const float4* s4 = (const float4*)src;
      float4* d4 = (float4*)dst;
      for (int e = threadIdx.x; e < D4; e += 256) d4[e] = src != nullptr ? s4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int e = threadIdx.x; e < D; e += 256) dst[e] = src != nullptr ? src[e] : 0.f;
    }
  }
  if (blockIdx.x == 0) {
    uint8_t* m = a.mask + (size_t)b * T_out;
    for (int t = threadIdx.x; t < T_out; t += 256) {
      uint8_t v = 0;
      if (t < keep) {
        v = a.mask_rgb != nullptr ? a.mask_rgb[(size_t)b * a.T_rgb + t] : (uint8_t)1;
      } else if (t < n) {
        v = a.mask_motion != nullptr ? a.mask_motion[(size_t)b * a.T_motion + (t - keep)] : (uint8_t)1;
      }
      m[t] = v;
    }
    if (b == 0 && threadIdx.x == 0) *a.pool_len = n;
  }
}

extern "C" int vmc_concat_tokens_len(const float* rgb, const float* motion, const uint8_t* mask_rgb, const uint8_t* mask_motion,
                                     float* x, uint8_t* mask, int* pool_len, int B, int T_rgb, int T_motion, int T_out, int D,
                                     const int* len_rgb, const int* len_motion, void* stream) {
  if (!rgb || !motion || !x || !mask || !pool_len) return VMC_E_ARG;
  if (B <= 0 || T_rgb <= 0 || T_motion <= 0 || T_out <= 0 || D <= 0 || B > 65535) return VMC_E_SHAPE;
  CtArgs a = {};
  a.rgb = rgb;
  a.motion = motion;
  a.mask_rgb = mask_rgb;
  a.mask_motion = mask_motion;
  a.x = x;
  a.mask = mask;
  a.pool_len = pool_len;
  a.len_rgb = len_rgb;
  a.len_motion = len_motion;
  a.B = B;
  a.T_rgb = T_rgb;
  a.T_motion = T_motion;
  a.T_out = T_out;
  a.D = D;
  a.vec = D % 4 == 0 && (((uintptr_t)rgb | (uintptr_t)motion | (uintptr_t)x) & 15) == 0;
  const dim3 grid((unsigned)((T_out + CT_ROWS - 1) / CT_ROWS), (unsigned)B);
  hipLaunchKernelGGL(concat_tokens_len_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- backward: the scatter of dx [B, T_out, D] back to the two streams ------------------------------------------------------------------
//   d rgb[b, t]    = dx[b, t]         for t < keep,  0 on rows keep..T_rgb-1 (the dropped last RGB row and the padding)
//   d motion[b, t] = dx[b, keep + t]  for t < nm,    0 on rows nm..T_motion-1
// with keep / nm clamped exactly as in the forward, from the same device values.  Every output row has ONE source row (or none), so
// it is one pass of plain vector stores: no atomics, and every element of both gradients is written on every call.
//   grid = (ceil(max(T_rgb, T_motion) / CT_ROWS), B, 2): z = 0 writes d rgb, z = 1 d motion; a workgroup owns CT_ROWS rows of one clip.
// BOUNDS: a destination row is < T_rgb (z = 0) or < T_motion (z = 1); a source row is < keep <= T_out or keep + t < keep + nm <= T_out.
struct CtBwdArgs {
  const float* dx;
  float* drgb;
  float* dmotion;
  const int* len_rgb;
  const int* len_motion;
  int B, T_rgb, T_motion, T_out, D;
  int vec;        // 16-byte path: D % 4 == 0, dx, drgb and dmotion 16-byte aligned
};

__global__ void __launch_bounds__(256) concat_tokens_len_bwd_kernel(const CtBwdArgs a) {
  const int b = blockIdx.y, T_out = a.T_out, D = a.D;
  int nr = a.len_rgb != nullptr ? *a.len_rgb : a.T_rgb;
  int nm = a.len_motion != nullptr ? *a.len_motion : a.T_motion;
  nr = nr < 1 ? 1 : (nr > a.T_rgb ? a.T_rgb : nr);
  nm = nm < 1 ? 1 : (nm > a.T_motion ? a.T_motion : nm);
  const int keep = nr - 1 < T_out ? nr - 1 : T_out;
  nm = nm < T_out - keep ? nm : T_out - keep;

  const bool mot = blockIdx.z == 1;
  const int T_dst = mot ? a.T_motion : a.T_rgb, n_src = mot ? nm : keep, s0 = mot ? keep : 0;
  float* dst_base = mot ? a.dmotion : a.drgb;
  const int t0 = blockIdx.x * CT_ROWS;
  const int t1 = t0 + CT_ROWS < T_dst ? t0 + CT_ROWS : T_dst;
  for (int t = t0; t < t1; ++t) {
    const float* src = t < n_src ? a.dx + ((size_t)b * T_out + s0 + t) * D : nullptr;      // nullptr: a zero row
    float* dst = dst_base + ((size_t)b * T_dst + t) * D;
    if (a.vec) {
      const int D4 = D >> 2;
      const float4* s4 = (const float4*)src;
      float4* d4 = (float4*)dst;
      for (int e = threadIdx.x; e < D4; e += 256) d4[e] = src != nullptr ? s4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int e = threadIdx.x; e < D; e += 256) dst[e] = src != nullptr ? src[e] : 0.f;
    }
  }
}

extern "C" int vmc_concat_tokens_len_bwd(const float* dx, float* drgb, float* dmotion, int B, int T_rgb, int T_motion, int T_out, int D,
                                         const int* len_rgb, const int* len_motion, void* stream) {
  if (!dx || !drgb || !dmotion) return VMC_E_ARG;
  if (B <= 0 || T_rgb <= 0 || T_motion <= 0 || T_out <= 0 || D <= 0 || B > 65535) return VMC_E_SHAPE;
  CtBwdArgs a = {};
  a.dx = dx;
  a.drgb = drgb;
  a.dmotion = dmotion;
  a.len_rgb = len_rgb;
  a.len_motion = len_motion;
  a.B = B;
  a.T_rgb = T_rgb;
  a.T_motion = T_motion;
  a.T_out = T_out;
  a.D = D;
  a.vec = D % 4 == 0 && (((uintptr_t)dx | (uintptr_t)drgb | (uintptr_t)dmotion) & 15) == 0;
  const int T_max = T_rgb > T_motion ? T_rgb : T_motion;
  const dim3 grid((unsigned)((T_max + CT_ROWS - 1) / CT_ROWS), (unsigned)B, 2);
  hipLaunchKernelGGL(concat_tokens_len_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  VMC_CHECK_LAUNCH();
  return 0;
}
