// K18 -- device-resident epoch log (gfx950): what the TFAM loops keep per step for the epoch's loss and metric (the logits rows, the
// label rows, torchmetrics' "this update call had a value outside [0, 1]" decision and the running loss), appended at a cursor that
// lives in device memory, so a captured step logs itself and the host reads once per epoch (include/vmc.h K18).
//
// Pure data movement: 4 B read and 5 B written per element, 1 120 elements (10 KB) at the reference batch (8 x 140).
//   ONE launch, ONE workgroup of 1024 threads, 4-byte lanes.
//   * The destination offset rows * C is a device value: its alignment is unknown to the host, so there is no 16-byte path.
//   * The squash flag belongs to the whole call and the cursor is read and advanced by the same call.  With one workgroup both
//     are workgroup-local: a ballot per wave, one LDS word per wave, one barrier.  More workgroups would need a second launch (or
//     scratch the ABI does not have) to agree on the flag; the step this feeds is launch bound (~1 ms of ~4 us launches), so the
//     second launch would cost more than the copy.  A large call (B = 4096: 573 440 elements, 5 MB) is 560 trips per thread.
//   * Every thread reads the cursor at kernel start; thread 0 alone writes the counters, with ordinary stores, after the barrier
//     behind which no thread reads them any more.  No atomics: the same bits on every replay.
//
// BOUNDS.  `state` is device memory the host cannot validate: rows < 0 or rows + B > capacity (64-bit) refuses the call before any
// address is formed from it -- status bit 1, nothing else written.  Otherwise rows + B <= capacity bounds every index below.
#include "common.h"

#define ML_THREADS 1024
#define ML_WAVES (ML_THREADS / 64)

__global__ void __launch_bounds__(ML_THREADS) metric_append_kernel(const vmc_metric_log log, const float* __restrict__ values,
                                                                   const float* __restrict__ targets, const float* __restrict__ loss,
                                                                   const int B) {
  __shared__ int s_out[ML_WAVES], s_bad[ML_WAVES];
  const int tid = threadIdx.x;
  const int rows = log.state[0];
  if (rows < 0 || (long long)rows + B > (long long)log.capacity) {      // uniform: every thread read the same word
    if (tid == 0) log.state[2] |= 1;
    return;
  }
  const long long n = (long long)B * log.C;
  const long long base = (long long)rows * log.C;
  float* __restrict__ dv = log.values + base;
  uint8_t* __restrict__ dt = log.targets + base;
  bool out = false, bad = false;
  for (long long e = tid; e < n; e += ML_THREADS) {
    const float v = values[e];
    dv[e] = v;
    out |= (v < 0.0f) | (v > 1.0f);                   // IEEE compares: false for NaN, -0.0, 0.0 and 1.0
    const float t = truncf(targets[e]);               // labels.to(torch.int): toward zero
    bad |= !(t == 0.0f || t == 1.0f);                 // NaN counts as "not a label" and is stored as 0
    dt[e] = t >= 255.0f ? (uint8_t)255 : (t >= 1.0f ? (uint8_t)(int)t : (uint8_t)0);
  }
  const bool w_out = __ballot(out) != 0ull, w_bad = __ballot(bad) != 0ull;
  if ((tid & 63) == 0) {
    s_out[tid >> 6] = w_out;
    s_bad[tid >> 6] = w_bad;
  }
  __syncthreads();
  int f = 0, any_bad = 0;
#pragma unroll
  for (int w = 0; w < ML_WAVES; ++w) {
    f |= s_out[w];
    any_bad |= s_bad[w];
  }
  uint8_t* __restrict__ ds = log.squash + rows;
  for (int r = tid; r < B; r += ML_THREADS) ds[r] = (uint8_t)f;
  if (tid == 0) {
    if (any_bad) log.state[2] |= 2;
    if (loss != nullptr) *log.loss_sum += *loss;
    log.state[1] += 1;
    log.state[0] = rows + B;
  }
}

extern "C" int vmc_metric_append(const vmc_metric_log* log, const float* values, const float* targets, const float* loss, int B,
                                 void* stream) {
  if (!log || !values || !targets || B <= 0) return VMC_E_ARG;
  if (!log->values || !log->targets || !log->squash || !log->state || !log->loss_sum || log->capacity <= 0 || log->C <= 0)
    return VMC_E_ARG;
  hipLaunchKernelGGL(metric_append_kernel, dim3(1), dim3(ML_THREADS), 0, (hipStream_t)stream, *log, values, targets, loss, B);
  VMC_CHECK_LAUNCH();
  return 0;
}
