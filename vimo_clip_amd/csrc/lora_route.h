// LoRA adapter kernels (lora.hip) as pure functions: argument validation, rank tiles, rows per workgroup and K chunk of
// vmc_lora_down_concat, and the column tiles / token slices / workspace of vmc_lora_wgrad_tn.  No HIP types: the launchers in
// lora.hip execute these plans, and tests/host/test_lora_route.cpp (plain g++) pins them.  DESIGN.md §3.3.4.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vmc.h"

constexpr int LORA_TAIL = 64;            // columns the adapter term occupies behind the K (or N) columns of a concat buffer
constexpr int LORA_CUS = 256;

// ---- vmc_lora_down_concat -------------------------------------------------------------------------------------------------------
// lora_down_kernel<T, NT, RT>: 256 threads, every wave owns RT tiles of 16 rows, NT = ceil(r / 16) rank tiles of the adapter; the
// adapter is staged in LDS kc columns at a time, rows padded by 8 elements ([16 NT][kc + 8]).
constexpr int LORA_DOWN_ROWS = 64;       // rows of one row tile of a workgroup (four waves x 16)
constexpr int LORA_DOWN_MAX_RT = 2;

struct LoraDownPlan {
  int rc;                // 0 or VMC_E_*
  int nt, rt;            // kernel instantiation
  int kc;                // adapter columns per LDS chunk (a multiple of 64)
  int rows_per_wg;       // 64 rt
  unsigned grid;
  int lds;               // dynamic LDS bytes
};

inline int lora_check_down(uintptr_t x, uintptr_t a16, uintptr_t out, long long ldx, long long lda, long long ldo, int M, int K, int r,
                           int col0) {
  if (!x || !a16 || !out) return VMC_E_ARG;
  if (M < 1 || K < 64 || K % 64 || r < 8 || r > LORA_TAIL || r % 8 || col0 < K || col0 % 8) return VMC_E_SHAPE;
  if (ldx < K || lda < K || ldo < (long long)col0 + LORA_TAIL) return VMC_E_SHAPE;
  if ((x | a16 | out) % 16 || ldx % 8 || lda % 8 || ldo % 8) return VMC_E_ALIGN;
  return 0;
}

inline LoraDownPlan lora_route_down(int M, int K, int r) {
  LoraDownPlan p = {};
  if (M < 1 || K < 64 || K % 64 || r < 8 || r > LORA_TAIL || r % 8) { p.rc = VMC_E_SHAPE; return p; }
  p.nt = (r + 15) / 16;
  // two row tiles per wave halve the adapter refills, but only while two workgroups per CU remain
  p.rt = ((long long)M + 2 * LORA_DOWN_ROWS - 1) / (2 * LORA_DOWN_ROWS) >= 2 * LORA_CUS ? 2 : 1;
  p.rows_per_wg = LORA_DOWN_ROWS * p.rt;
  const int kc_max = p.nt <= 2 ? 512 : 256;          // at most 33 KiB + padding: four workgroups per CU
  p.kc = K < kc_max ? K : kc_max;
  p.grid = (unsigned)(((long long)M + p.rows_per_wg - 1) / p.rows_per_wg);
  p.lds = 16 * p.nt * (p.kc + 8) * 2;
  return p;
}

// ---- vmc_lora_wgrad_tn ----------------------------------------------------------------------------------------------------------
// lora_wgrad_kernel<T, NT, TR>: 256 threads, one 128-column tile of x against all r columns of t over one token slice, staged 64
// tokens at a time; partial sums go to fp32 slabs that lora_slab_sum_kernel adds in slice order (one slice: straight to out).
constexpr int LORA_WG_COLS = 128;
constexpr int LORA_WG_TOKENS = 64;
constexpr int LORA_WG_MIN_SLICE = 256;   // fewest tokens a slice is planned with
constexpr int LORA_WG_MAX_SLICES = 256;

struct LoraWgradPlan {
  int rc;
  int nt;                // rank tiles of 16
  int c_tiles;
  int slices, tokens_per_slice;      // tokens_per_slice is a multiple of 64; the last slice may be shorter
  size_t workspace_bytes;            // 0 with one slice
};

inline LoraWgradPlan lora_route_wgrad(int M, int r, int C) {
  LoraWgradPlan p = {};
  if (M < 1 || r < 8 || r > LORA_TAIL || r % 8 || C < 8 || C % 8) { p.rc = VMC_E_SHAPE; return p; }
  p.nt = (r + 15) / 16;
  p.c_tiles = (C + LORA_WG_COLS - 1) / LORA_WG_COLS;
  int want = (2 * LORA_CUS + p.c_tiles - 1) / p.c_tiles;                    // two workgroups per CU
  const int most = (M + LORA_WG_MIN_SLICE - 1) / LORA_WG_MIN_SLICE;
  if (want > most) want = most;
  if (want > LORA_WG_MAX_SLICES) want = LORA_WG_MAX_SLICES;
  if (want < 1) want = 1;
  const int per = (M + want - 1) / want;
  p.tokens_per_slice = (per + LORA_WG_TOKENS - 1) / LORA_WG_TOKENS * LORA_WG_TOKENS;
  p.slices = (M + p.tokens_per_slice - 1) / p.tokens_per_slice;
  p.workspace_bytes = p.slices > 1 ? (size_t)p.slices * r * C * sizeof(float) : 0;
  return p;
}

inline int lora_check_wgrad(uintptr_t t, uintptr_t x, uintptr_t out, long long ldt, long long ldx, int M, int r, int C, uintptr_t workspace,
                            size_t workspace_bytes) {
  if (!t || !x || !out) return VMC_E_ARG;
  const LoraWgradPlan p = lora_route_wgrad(M, r, C);
  if (p.rc) return p.rc;
  if (ldt < r || ldx < C) return VMC_E_SHAPE;
  if (p.workspace_bytes && (!workspace || workspace_bytes < p.workspace_bytes)) return VMC_E_ARG;
  if ((t | x | out) % 16 || ldt % 8 || ldx % 8 || (p.workspace_bytes && workspace % 16)) return VMC_E_ALIGN;
  return 0;
}
