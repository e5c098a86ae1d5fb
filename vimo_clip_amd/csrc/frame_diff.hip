// Frame-difference motion frames from RGB frames (gfx950): out[t] = |gray(f[t+1]) - gray(f[t])|, the arithmetic of the
// reference's utils/generate_frame_diff_video.py (cv2.cvtColor(COLOR_BGR2GRAY) + cv2.absdiff) before its lossy encode.
//
// HBM bound: per output pixel 3 B are read (each input frame feeds TWO outputs, but is fetched once) and channels_out B written.
//   * one thread owns FD_PX = 4 consecutive pixels of one row and WALKS TIME: the grey values of the previous frame stay in
//     registers, so a frame is fetched once per time segment, not once per output that needs it;
//   * accesses are 4 bytes per lane where the layout allows: three u32 loads cover the 12 bytes of four packed RGB pixels
//     (stride_x == 3, stride_c == 1) or four pixels of each plane (stride_x == 1), one u32 store writes four outputs.  The
//     vector form is chosen PER THREAD AND PER ACCESS from the address itself (4 whole pixels inside the row and a 4-byte aligned
//     address), so unaligned rows, odd pitches, ragged row ends and every other stride pattern take the byte path of the same
//     expression and give the same bytes.
//
// Time segments.  A (row, 4-pixel group) thread alone gives H * ceil(W/4) threads, 57.6 k for a 360 x 640 frame: a ninth of the
// 256 CUs x 2048 resident threads.  The output frames are therefore split into ceil(n_out / L) segments on gridDim.y, each of
// which re-reads ONE frame (its first) that the previous segment also read: the read traffic grows by 1/L.  L is the SMALLEST
// split that fills the machine and never shorter than VMC_FRAME_DIFF_MIN_SEG = 8 (re-read <= 12.5 % of the reads, 9 % of all
// bytes at one output channel):
//     L = max(8, ceil(n_out / ceil(256 * 2048 / threads_per_frame))), capped at n_out.
// 256 frames of 360 x 640: 10 segments of 26 outputs (9 frames read twice: +3.5 % reads); small frames get L = 8; frames of
// >= 524 k groups are never split.  None of this has been tuned against a measurement: tools/frame_diff_bench.py records what
// this choice gives.
#include "common.h"

#define FD_PX 4
#define FD_FILL_THREADS (256 * 2048)

enum { FD_GENERIC = 0, FD_PACKED = 1, FD_PLANAR = 2 };

struct FdWeights {
  uint32_t r, g, b, round;
  int shift;
};

__device__ __forceinline__ uint32_t fd_gray(uint32_t r, uint32_t g, uint32_t b, const FdWeights& w) {
  return (w.r * r + w.g * g + w.b * b + w.round) >> w.shift;      // <= 255 * 2^shift + 2^(shift-1) < 2^31 for shift <= 22
}

// Grey values of the n (1..4) pixels that start at p (the R byte of pixel x of one row).
template <int LAYOUT>
__device__ __forceinline__ void fd_load_gray(const uint8_t* __restrict__ p, int n, long long sc, long long sx, const FdWeights& w,
                                             uint32_t g[FD_PX]) {
  if (LAYOUT == FD_PACKED && n == FD_PX && ((uintptr_t)p & 3) == 0) {
    const uint32_t a = ((const uint32_t*)p)[0], b = ((const uint32_t*)p)[1], c = ((const uint32_t*)p)[2];      // RGBR GBRG BRGB
    g[0] = fd_gray(a & 0xFFu, (a >> 8) & 0xFFu, (a >> 16) & 0xFFu, w);
    g[1] = fd_gray(a >> 24, b & 0xFFu, (b >> 8) & 0xFFu, w);
    g[2] = fd_gray((b >> 16) & 0xFFu, b >> 24, c & 0xFFu, w);
    g[3] = fd_gray((c >> 8) & 0xFFu, (c >> 16) & 0xFFu, c >> 24, w);
    return;
  }
  if (LAYOUT == FD_PLANAR && n == FD_PX && (((uintptr_t)p | (uintptr_t)sc) & 3) == 0) {
    const uint32_t r = *(const uint32_t*)p, gg = *(const uint32_t*)(p + sc), b = *(const uint32_t*)(p + 2 * sc);
#pragma unroll
    for (int j = 0; j < FD_PX; ++j) g[j] = fd_gray((r >> (8 * j)) & 0xFFu, (gg >> (8 * j)) & 0xFFu, (b >> (8 * j)) & 0xFFu, w);
    return;
  }
#pragma unroll
  for (int j = 0; j < FD_PX; ++j) {
    if (j < n) {
      const uint8_t* q = p + j * sx;
      g[j] = fd_gray(q[0], q[sc], q[2 * sc], w);
    } else {
      g[j] = 0;
    }
  }
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) frame_diff_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ prev,
                                                         uint8_t* __restrict__ out, int H, int W, long long st, long long sc,
                                                         long long sy, long long sx, FdWeights w, int channels_out, int n_out,
                                                         int seg_len) {
  const int groups_per_row = (W + FD_PX - 1) / FD_PX;
  const size_t gidx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gidx >= (size_t)H * groups_per_row) return;
  const int y = (int)(gidx / groups_per_row);
  const int x = (int)(gidx % groups_per_row) * FD_PX;
  const int n = W - x < FD_PX ? W - x : FD_PX;
  const int o0 = blockIdx.y * seg_len;
  const int o1 = o0 + seg_len < n_out ? o0 + seg_len : n_out;
  const int has_prev = prev != nullptr;
  const long long pix = (long long)y * sy + (long long)x * sx;
  // f[s], s = 0 .. n_out: `prev` first when it is given, then frames[0 .. T-1]
  auto frame = [&](int s) -> const uint8_t* { return (has_prev && s == 0) ? prev + pix : frames + (long long)(s - has_prev) * st + pix; };
  const size_t plane = (size_t)H * W;
  uint8_t* dst = out + (size_t)o0 * channels_out * plane + (size_t)y * W + x;
  uint32_t last[FD_PX], cur[FD_PX];
  fd_load_gray<LAYOUT>(frame(o0), n, sc, sx, w, last);
#pragma unroll 2
  for (int o = o0; o < o1; ++o) {
    fd_load_gray<LAYOUT>(frame(o + 1), n, sc, sx, w, cur);
    uint32_t d[FD_PX];
#pragma unroll
    for (int j = 0; j < FD_PX; ++j) {
      d[j] = cur[j] > last[j] ? cur[j] - last[j] : last[j] - cur[j];
      last[j] = cur[j];
    }
    const uint32_t packed = d[0] | (d[1] << 8) | (d[2] << 16) | (d[3] << 24);
    for (int c = 0; c < channels_out; ++c) {
      uint8_t* q = dst + c * plane;
      if (n == FD_PX && ((uintptr_t)q & 3) == 0) {
        *(uint32_t*)q = packed;
      } else {
#pragma unroll
        for (int j = 0; j < FD_PX; ++j)
          if (j < n) q[j] = (uint8_t)d[j];
      }
    }
    dst += (size_t)channels_out * plane;
  }
}

extern "C" int vmc_frame_diff_gray_u8(const uint8_t* frames, const uint8_t* prev, uint8_t* out, int T, int H, int W,
                                      long long stride_t, long long stride_c, long long stride_y, long long stride_x, int w_r, int w_g,
                                      int w_b, int shift, int channels_out, void* stream) {
  if (!frames || !out || T <= 0 || H <= 0 || W <= 0) return VMC_E_ARG;
  const int n_out = T - 1 + (prev != nullptr);
  if (n_out <= 0) return VMC_E_ARG;
  if (channels_out != 1 && channels_out != 3) return VMC_E_ARG;
  if (shift < 1 || shift > 22 || w_r < 0 || w_g < 0 || w_b < 0) return VMC_E_ARG;
  if ((long long)w_r + w_g + w_b != (1ll << shift)) return VMC_E_ARG;          // the sum rule keeps grey <= 255
  const size_t groups = (size_t)H * ((W + FD_PX - 1) / FD_PX);
  const size_t blocks = (groups + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return VMC_E_SHAPE;
  const size_t want = (FD_FILL_THREADS + groups - 1) / groups;                  // segments that fill the machine
  int seg_len = (int)(((size_t)n_out + want - 1) / want);
  if (seg_len < VMC_FRAME_DIFF_MIN_SEG) seg_len = VMC_FRAME_DIFF_MIN_SEG;
  if (seg_len > n_out) seg_len = n_out;
  const int nseg = (n_out + seg_len - 1) / seg_len;
  if (nseg > 65535) return VMC_E_SHAPE;
  const FdWeights w = {(uint32_t)w_r, (uint32_t)w_g, (uint32_t)w_b, 1u << (shift - 1), shift};
  const dim3 grid((unsigned)blocks, (unsigned)nseg);
  hipStream_t s = (hipStream_t)stream;
  if (stride_x == 3 && stride_c == 1)
    hipLaunchKernelGGL(frame_diff_kernel<FD_PACKED>, grid, dim3(256), 0, s, frames, prev, out, H, W, stride_t, stride_c, stride_y, stride_x, w,
                       channels_out, n_out, seg_len);
  else if (stride_x == 1)
    hipLaunchKernelGGL(frame_diff_kernel<FD_PLANAR>, grid, dim3(256), 0, s, frames, prev, out, H, W, stride_t, stride_c, stride_y, stride_x, w,
                       channels_out, n_out, seg_len);
  else
    hipLaunchKernelGGL(frame_diff_kernel<FD_GENERIC>, grid, dim3(256), 0, s, frames, prev, out, H, W, stride_t, stride_c, stride_y, stride_x, w,
                       channels_out, n_out, seg_len);
  VMC_CHECK_LAUNCH();
  return 0;
}
