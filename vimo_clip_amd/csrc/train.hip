// Losses (value + gradient in one pass) and the fused Adam/AdamW update (gfx950, fp32, HBM-bound).
#include "common.h"
#include "grad_sumsq.h"

// ---- distillation loss (losses.py:5-44) ---------------------------------------------------------
// One wave per row.  Cosine: ns = max(|s|, eps), nt = max(|t|, eps), c = clamp(s.t/(ns nt), +-(1-eps)),
// loss = mean(1 - c).  d loss / d s = -(1/rows) * [ t/(ns nt) - (s.t) s / (ns^3 nt) * 1{|s| > eps} ] * 1{c not clamped}.
// Row partial losses go to the workspace; a single-block kernel sums them in a fixed order.
__global__ void __launch_bounds__(256) distill_rows_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                           float* __restrict__ row_loss, float* __restrict__ ds, int rows, int E,
                                                           int rows_per_clip, size_t teacher_clip_stride, int cosine) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* sr = s + (size_t)row * E;
  const float* tr = t + (size_t)(row / rows_per_clip) * teacher_clip_stride + (size_t)(row % rows_per_clip) * E;
  const float eps = 1e-5f;
  if (cosine) {
    float dot = 0.f, ss = 0.f, tt = 0.f;
    for (int i = lane; i < E; i += 64) {
      const float a = sr[i], b = tr[i];
      dot += a * b; ss += a * a; tt += b * b;
    }
    dot = wave_sum(dot); ss = wave_sum(ss); tt = wave_sum(tt);
    const float sn_raw = sqrtf(ss), tn_raw = sqrtf(tt);
    const float sn = fmaxf(sn_raw, eps), tn = fmaxf(tn_raw, eps);
    const float c_raw = dot / (sn * tn);
    const float c = fminf(fmaxf(c_raw, -1.0f + eps), 1.0f - eps);
    if (lane == 0) row_loss[row] = 1.0f - c;
    if (ds) {
      // torch.clamp passes gradient on the closed interval [min, max]
      const bool pass = (c_raw >= -1.0f + eps) && (c_raw <= 1.0f - eps);
      const float k = pass ? -1.0f / (float)rows : 0.0f;
      const float inv = 1.0f / (sn * tn);
      // norm clamp(min=eps) passes gradient when |s| >= eps; d|s|/ds = s/|s| (0 at s = 0)
      const float kn = (sn_raw >= eps && sn_raw > 0.f) ? dot / (sn * sn * tn * sn_raw) : 0.0f;
      for (int i = lane; i < E; i += 64) ds[(size_t)row * E + i] = k * (tr[i] * inv - sr[i] * kn);
    }
  } else {
    float acc = 0.f;
    const float k = 2.0f / ((float)rows * (float)E);
    for (int i = lane; i < E; i += 64) {
      const float d = sr[i] - tr[i];
      acc += d * d;
      if (ds) ds[(size_t)row * E + i] = k * d;
    }
    acc = wave_sum(acc);
    if (lane == 0) row_loss[row] = acc / (float)E;
  }
}

__global__ void __launch_bounds__(256) sum_scale_kernel(const float* __restrict__ part, float* __restrict__ out, int n, float scale) {
  __shared__ float sm[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((sm[0] + sm[1]) + (sm[2] + sm[3])) * scale;
}

extern "C" size_t vmc_loss_workspace_bytes(int rows) { return (size_t)(rows > 0 ? rows : 1) * sizeof(float); }

extern "C" int vmc_distill_loss(const float* student, const float* teacher, float* loss, float* dstudent, int rows, int E,
                                int rows_per_clip, size_t teacher_clip_stride, int mode_cosine, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!student || !teacher || !loss || !workspace || rows <= 0 || E <= 0 || rows_per_clip <= 0) return VMC_E_ARG;
  if (workspace_bytes < vmc_loss_workspace_bytes(rows)) return VMC_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(distill_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, student, teacher, (float*)workspace, dstudent, rows, E,
                     rows_per_clip, teacher_clip_stride, mode_cosine);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, loss, rows, 1.0f / (float)rows);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- BCE with logits, pos_weight = pw*y + 1 (losses.py:59-67) ------------------------------------
// l = (1-y) x + (1 + (w-1) y) (log1p(exp(-|x|)) + max(-x, 0));  dl/dx = (1-y) sigmoid(x) - w y sigmoid(-x), each sigmoid from
// e = exp(-|x|) without a subtraction (1 / (1 + e) or e / (1 + e)): (1-y) - lw (1 - sigmoid(x)) cancels in both confident tails
// (relative error 1e-4 at |x| = 9, 2e-3 at 13, a gradient of exactly 0 from |x| = 17).
#define BCE_BLOCKS 64
__global__ void __launch_bounds__(256) bce_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ part,
                                                  float* __restrict__ dx, int n, float pw, float* __restrict__ loss_out) {
  __shared__ float sm[4];
  float acc = 0.f;
  const float invn = 1.0f / (float)n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float xi = x[i], yi = y[i];
    const float w = pw < 0.f ? 1.0f : pw * yi + 1.0f;
    const float lw = 1.0f + (w - 1.0f) * yi;
    const float e = expf(-fabsf(xi));
    acc += (1.0f - yi) * xi + lw * (log1pf(e) + fmaxf(-xi, 0.0f));
    if (dx) {
      const float r = 1.0f / (1.0f + e);
      const float sig_pos = xi >= 0.f ? r : e * r, sig_neg = xi >= 0.f ? e * r : r;      // sigmoid(x), sigmoid(-x)
      dx[i] = ((1.0f - yi) * sig_pos - (w * yi) * sig_neg) * invn;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    if (loss_out != nullptr) loss_out[0] = tot * invn;      // single-workgroup launch (small n): no second pass
    else part[blockIdx.x] = tot;
  }
}

extern "C" int vmc_bce_loss(const float* logits, const float* targets, float* loss, float* dlogits, int n, float pos_weight,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits || !targets || !loss || !workspace || n <= 0) return VMC_E_ARG;
  if (workspace_bytes < BCE_BLOCKS * sizeof(float)) return VMC_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  int blocks = (n + 255) / 256;
  if (blocks > BCE_BLOCKS) blocks = BCE_BLOCKS;
  if (n <= 8192) {      // a TFAM batch of a few clips x 140 classes: one workgroup, one launch (the launch count is the cost there)
    hipLaunchKernelGGL(bce_kernel, dim3(1), dim3(256), 0, s, logits, targets, (float*)workspace, dlogits, n, pos_weight, loss);
    VMC_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(bce_kernel, dim3(blocks), dim3(256), 0, s, logits, targets, (float*)workspace, dlogits, n, pos_weight, (float*)nullptr);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, loss, blocks, 1.0f / (float)n);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- softmax cross entropy (nn.CrossEntropyLoss, mean over rows) ------------------------------------
// One wave per row: m = max x, se = sum exp(x - m).  Index targets: l = log(se) - (x[t] - m).  Probability targets
// (float [rows, C], what the MammalNet TFAM loop passes): l = sum(y) log(se) - sum_c y_c (x_c - m).  d l / d x_c = softmax_c * sum(y) - y_c.
// The loss never passes through lse = m + log(se): a confident row's small loss would be rounded at the size of m (logits
// [80, 68.5, 0], target 0: 7.6e-6 for 1.013e-5).
__global__ void __launch_bounds__(256) ce_rows_kernel(const float* __restrict__ x, const long long* __restrict__ tidx,
                                                      const float* __restrict__ tprob, float* __restrict__ row_loss,
                                                      float* __restrict__ dx, int rows, int C) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + (size_t)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  float se = 0.f, ysum = 0.f, yx = 0.f;      // yx = sum_c y_c (x_c - m)
  for (int c = lane; c < C; c += 64) {
    const float xm = xr[c] - m;
    se += expf(xm);
    if (tprob) {
      const float y = tprob[(size_t)row * C + c];
      ysum += y;
      yx += y * xm;
    }
  }
  se = wave_sum(se);
  long long t = -1;
  if (tprob) {
    ysum = wave_sum(ysum);
    yx = wave_sum(yx);
  } else {
    t = tidx[row];
    ysum = 1.0f;
    yx = (t >= 0 && t < C) ? xr[t] - m : -m;      // an index outside [0, C) leaves lse, as before
  }
  if (lane == 0) row_loss[row] = ysum * logf(se) - yx;
  if (dx) {
    const float inv = 1.0f / (float)rows, rse = 1.0f / se;
    for (int c = lane; c < C; c += 64) {
      const float y = tprob ? tprob[(size_t)row * C + c] : (c == t ? 1.0f : 0.0f);
      dx[(size_t)row * C + c] = (expf(xr[c] - m) * rse * ysum - y) * inv;
    }
  }
}

extern "C" int vmc_cross_entropy_loss(const float* logits, const long long* target_index, const float* target_prob, float* loss,
                                      float* dlogits, int rows, int C, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits || !loss || !workspace || rows <= 0 || C <= 0) return VMC_E_ARG;
  if ((target_index == nullptr) == (target_prob == nullptr)) return VMC_E_ARG;       // exactly one kind of target
  if (workspace_bytes < vmc_loss_workspace_bytes(rows)) return VMC_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ce_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, target_index, target_prob, (float*)workspace, dlogits, rows, C);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, loss, rows, 1.0f / (float)rows);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- fused Adam / AdamW ---------------------------------------------------------------------------
// 16 B read (p, g, m, v) + 12 B write per parameter; float4 vectorised, grid-stride.
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                                   float wd, int decoupled, float step_size, float inv_sqrt_bc2, float gscale,
                                                   const float* __restrict__ hyper, const int* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;      // a skipped step (vmc_loss_scale_check found inf / NaN): uniform, before any store
  if (hyper != nullptr) {      // captured training step: {lr, lr / (1 - b1^t), 1 / sqrt(1 - b2^t), grad_scale} live in device memory
    lr = hyper[0]; step_size = hyper[1]; inv_sqrt_bc2 = hyper[2]; gscale = hyper[3];
  }
  const size_t n4 = n >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  // two float4 of each of the four streams in flight per thread: a grid of 2 workgroups per CU (what the backward-overlapped
  // step launches, so that the update never takes the wave slots the backward's workgroups need) still covers the HBM latency
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += 2 * stride) {
    const size_t i1 = i0 + stride;
    const bool two = i1 < n4;
    float4 pp[2], gg[2], mm[2], vv[2];
    pp[0] = ((float4*)p)[i0]; gg[0] = ((const float4*)g)[i0]; mm[0] = ((float4*)m)[i0]; vv[0] = ((float4*)v)[i0];
    if (two) { pp[1] = ((float4*)p)[i1]; gg[1] = ((const float4*)g)[i1]; mm[1] = ((float4*)m)[i1]; vv[1] = ((float4*)v)[i1]; }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float* P = &pp[u].x; const float* G = &gg[u].x; float* M = &mm[u].x; float* V = &vv[u].x;
#pragma unroll
      for (int j = 0; j < 4; ++j) adam_element(P[j], G[j], M[j], V[j], lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, gscale);
      const size_t i = u ? i1 : i0;
      ((float4*)p)[i] = pp[u]; ((float4*)m)[i] = mm[u]; ((float4*)v)[i] = vv[u];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t k = (n4 << 2) + threadIdx.x;
    float pk = p[k], mk = m[k], vk = v[k];
    adam_element(pk, g[k], mk, vk, lr, b1, b2, eps, wd, decoupled, step_size, inv_sqrt_bc2, gscale);
    p[k] = pk; m[k] = mk; v[k] = vk;
  }
}

extern "C" int vmc_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int decoupled_wd, int step, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || n == 0 || step <= 0) return VMC_E_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return VMC_E_ALIGN;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for((n + 3) / 4, 256, 256 * 8)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                     beta2, eps, weight_decay, decoupled_wd, step_size, inv_sqrt_bc2, grad_scale, (const float*)nullptr, (const int*)nullptr);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- device-resident step state (hipGraph-captured training steps) ------------------------------------------------------
// state[0] = step count t, state[1] = base seed, state[2 .. 2 + n_seeds) = the dropout seeds of this step (one per call site);
// hyper = {lr (host-written), lr / (1 - b1^t), 1 / sqrt(1 - b2^t), grad_scale (host-written)}.
__global__ void train_tick_kernel(unsigned long long* __restrict__ state, float* __restrict__ hyper, float b1, float b2, int n_seeds) {
  __shared__ unsigned long long t_sh;
  if (threadIdx.x == 0) {
    const unsigned long long t = state[0] + 1;
    state[0] = t;
    t_sh = t;
    const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
    hyper[1] = (float)((double)hyper[0] / bc1);
    hyper[2] = (float)(1.0 / sqrt(bc2));
  }
  __syncthreads();
  const unsigned long long t = t_sh, base = state[1];
  for (int i = threadIdx.x; i < n_seeds; i += blockDim.x) {
    unsigned long long x = base ^ (t * 0x9E3779B97F4A7C15ull + (unsigned long long)i * 0xD1B54A32D192ED03ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    state[2 + i] = x & ~VMC_SEED_IS_PTR;        // a seed VALUE never carries the pointer tag
  }
}

extern "C" int vmc_train_tick(void* state, float* hyper, float beta1, float beta2, int n_seeds, void* stream) {
  if (!state || !hyper || n_seeds < 0) return VMC_E_ARG;
  hipLaunchKernelGGL(train_tick_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)state, hyper, beta1, beta2, n_seeds);
  VMC_CHECK_LAUNCH();
  return 0;
}

extern "C" int vmc_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                                 float eps, float weight_decay, int decoupled_wd, void* stream) {
  return vmc_adam_step_dev_skip(p, g, m, v, n, hyper, beta1, beta2, eps, weight_decay, decoupled_wd, 256 * 8, nullptr, stream);
}
extern "C" int vmc_adam_step_dev_bg(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                                    float eps, float weight_decay, int decoupled_wd, int max_workgroups, void* stream) {
  return vmc_adam_step_dev_skip(p, g, m, v, n, hyper, beta1, beta2, eps, weight_decay, decoupled_wd, max_workgroups, nullptr, stream);
}
extern "C" int vmc_adam_step_dev_skip(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float beta1, float beta2,
                                      float eps, float weight_decay, int decoupled_wd, int max_workgroups, const int* skip, void* stream) {
  if (!p || !g || !m || !v || !hyper || n == 0 || max_workgroups <= 0) return VMC_E_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)hyper) & 15) return VMC_E_ALIGN;
  if ((uintptr_t)skip & 3) return VMC_E_ALIGN;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for((n + 3) / 4, 256, max_workgroups)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, 0.f, beta1,
                     beta2, eps, weight_decay, decoupled_wd, 0.f, 0.f, 0.f, hyper, skip);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- gradient clipping on the device (clip_grad_norm_ inside a captured step, train.py:105-106) -----------------------
// Store and sum (grad_sumsq.h, shared with vmc_loss_scale_check): pass one leaves one double per workgroup, pass two (one workgroup)
// adds them in a fixed order and writes clip[2..3] and hyper[3] (include/vmc.h).
__global__ void __launch_bounds__(256) grad_sumsq_partial_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double sm[4];
  unsigned bad = 0;
  double s = grad_sumsq_thread<false>(g, n, bad);
  s = block_sum_f64(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) grad_clip_finish_kernel(const double* __restrict__ part, int n_part, float* __restrict__ hyper,
                                                               float* __restrict__ clip) {
  __shared__ double sm[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += 256) s += part[i];
  s = block_sum_f64(s, sm);
  if (threadIdx.x == 0) {
    const float base = clip[0], max_norm = clip[1];
    const double norm = sqrt(s) * fabs((double)base);                  // of the AVERAGED gradient (optim.clipped_grad_scale)
    const float coef = grad_clip_coef(norm, max_norm);
    clip[2] = (float)norm;
    clip[3] = coef;
    hyper[3] = base * coef;
  }
}

extern "C" size_t vmc_grad_clip_workspace_bytes(size_t n) { return (size_t)grad_clip_blocks(n) * sizeof(double); }

extern "C" int vmc_grad_clip_dev(const float* grad, size_t n, float* hyper, float* clip, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (!grad || !hyper || !clip || !workspace || n == 0) return VMC_E_ARG;
  if (workspace_bytes < vmc_grad_clip_workspace_bytes(n)) return VMC_E_ARG;
  if (((uintptr_t)grad | (uintptr_t)hyper | (uintptr_t)clip | (uintptr_t)workspace) & 15) return VMC_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = grad_clip_blocks(n);
  hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(blocks), dim3(256), 0, s, grad, n, (double*)workspace);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, blocks, hyper, clip);
  VMC_CHECK_LAUNCH();
  return 0;
}

// ---- sum of squares (global grad-norm for clip_grad_norm_, train.py:105-106) ----------------------
__global__ void __launch_bounds__(256) sumsq_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
  __shared__ float sm[4];
  float a = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a += x[i] * x[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (sm[0] + sm[1]) + (sm[2] + sm[3]));
}
extern "C" int vmc_sumsq(const float* x, size_t n, float* out, void* stream) {
  if (!x || !out || n == 0) return VMC_E_ARG;
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, (hipStream_t)stream, x, n, out);
  VMC_CHECK_LAUNCH();
  return 0;
}
