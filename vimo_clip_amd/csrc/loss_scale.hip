// K21 — dynamic loss scaling on the device (include/vmc.h, optim.FusedAdam.enable_loss_scaling): torch.amp.GradScaler's unscale +
// found-inf check + update() as two launches over the flat gradient arena, with no host read, so a captured or no-sync step keeps
// its shape.  The scaler record (vmc_loss_scale_state) lives where the step count, the learning rate and the clip coefficient live.
//   pass 1  streams the arena once (4 B per parameter, 16-byte loads, the walk of vmc_grad_clip_dev: grad_sumsq.h) and leaves per
//           workgroup a double (sum of squares of its share) and an int (1 if any element it read is ±inf or NaN -- per ELEMENT,
//           not from the sum: a finite 1e20 is no overflow although its fp32 square is inf).
//   pass 2  one workgroup adds the partials in a fixed order, ORs the flags, and ONE thread makes every store: found_inf, the clip
//           norm / coefficient (of the UNSCALED averaged gradient: sqrt(sum) * |base_scale| / S), hyper[3] = base_scale / S * coef
//           (what the Adam kernels multiply the gradient with; 0 on overflow), torch._amp_update_scale_'s state machine, and on
//           overflow state[0] -= 1, which takes back the tick of this step.
// No atomics anywhere: the same gradient and the same record give the same bits on every call and every replay.
#include "common.h"
#include "grad_sumsq.h"

static_assert(sizeof(vmc_loss_scale_state) == 32, "vmc_loss_scale_state layout (include/vmc.h)");

__global__ void __launch_bounds__(256) loss_scale_partial_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part,
                                                                 int* __restrict__ flag) {
  __shared__ double sm[4];
  __shared__ unsigned bad_sh[4];
  unsigned bad = 0;
  double s = grad_sumsq_thread<true>(g, n, bad);
  const bool wave_bad = __any((int)bad);
  if ((threadIdx.x & 63) == 0) bad_sh[threadIdx.x >> 6] = wave_bad ? 1u : 0u;
  s = block_sum_f64(s, sm);                       // its barrier also publishes bad_sh
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    flag[blockIdx.x] = (int)(bad_sh[0] | bad_sh[1] | bad_sh[2] | bad_sh[3]);
  }
}

__global__ void __launch_bounds__(256) loss_scale_finish_kernel(const double* __restrict__ part, const int* __restrict__ flag, int n_part,
                                                                vmc_loss_scale_state* __restrict__ ls, float* __restrict__ hyper,
                                                                float* __restrict__ clip, unsigned long long* __restrict__ state) {
  __shared__ double sm[4];
  __shared__ unsigned bad_sh[4];
  double s = 0.0;
  unsigned bad = 0;
  for (int i = threadIdx.x; i < n_part; i += 256) {
    s += part[i];
    bad |= (unsigned)flag[i];
  }
  const bool wave_bad = __any((int)bad);
  if ((threadIdx.x & 63) == 0) bad_sh[threadIdx.x >> 6] = wave_bad ? 1u : 0u;
  s = block_sum_f64(s, sm);
  if (threadIdx.x != 0) return;
  const bool found = (bad_sh[0] | bad_sh[1] | bad_sh[2] | bad_sh[3]) != 0;
  const float S = ls->scale, base = ls->base_scale;
  float coef = 1.0f;
  if (clip != nullptr) {
    // norm of the unscaled AVERAGED gradient; with a power-of-two S the division is exact and coef has the bits of vmc_grad_clip_dev
    const double norm = sqrt(s) * fabs((double)base) / (double)S;
    coef = grad_clip_coef(norm, clip[1]);
    clip[2] = (float)norm;          // on overflow: the non-finite norm and whatever coefficient it gives, as vmc_grad_clip_dev
    clip[3] = coef;
  }
  ls->found_inf = found ? 1 : 0;
  hyper[3] = found ? 0.0f : base / S * coef;
  // torch._amp_update_scale_ (ATen/native/cuda/AmpKernels.cu, amp_update_scale_cuda_kernel)
  if (found) {
    ls->scale = S * ls->backoff_factor;
    ls->growth_tracker = 0;
    ls->skipped += 1;
    if (state != nullptr) state[0] -= 1;          // the skipped step does not count: the next tick recomputes the same t
  } else {
    const int successful = ls->growth_tracker + 1;
    if (successful == ls->growth_interval) {
      const float grown = S * ls->growth_factor;
      if ((__float_as_uint(grown) & 0x7f800000u) != 0x7f800000u) ls->scale = grown;
      ls->growth_tracker = 0;
    } else {
      ls->growth_tracker = successful;
    }
  }
}

// doubles first (8-byte aligned at the 16-byte aligned base), the flags behind them; rounded up to 16 bytes
extern "C" size_t vmc_loss_scale_workspace_bytes(size_t n) {
  return ((size_t)grad_clip_blocks(n) * (sizeof(double) + sizeof(int)) + 15) & ~(size_t)15;
}

extern "C" int vmc_loss_scale_check(const float* grad, size_t n, vmc_loss_scale_state* ls, float* hyper, float* clip, void* train_state,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad || !ls || !hyper || !workspace || n == 0) return VMC_E_ARG;
  if (workspace_bytes < vmc_loss_scale_workspace_bytes(n)) return VMC_E_ARG;
  if (((uintptr_t)grad | (uintptr_t)ls | (uintptr_t)hyper | (uintptr_t)clip | (uintptr_t)workspace) & 15) return VMC_E_ALIGN;
  if ((uintptr_t)train_state & 7) return VMC_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = grad_clip_blocks(n);
  double* part = (double*)workspace;
  int* flag = (int*)(part + blocks);
  hipLaunchKernelGGL(loss_scale_partial_kernel, dim3(blocks), dim3(256), 0, s, grad, n, part, flag);
  VMC_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_scale_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const int*)flag, blocks, ls, hyper, clip,
                     (unsigned long long*)train_state);
  VMC_CHECK_LAUNCH();
  return 0;
}
