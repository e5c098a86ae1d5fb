// Prints the plan vimo_clip_amd/csrc/gemm_route.h gives to each call described on stdin, one per line, so that
// tests/test_gemm_refs_host.py can hold every case of tests/gemm_refs.py to the kernel it is named for.  Built with g++ by that test.
//   linear M N K lda ldw ldc ldres ldz act bias res Z out_dtype res_dtype out_row_group res_row_mod dtype16 variant cfg ks u mfma32
//          (bias / res / Z: 0 = NULL, 1 = present; cfg ks u mfma32: the VMC_GEMM_CFG / _KS / _U / _MFMA32 switches)
//       -> rc | n {family cfg row0 rows} x n       family: TILE | G8 | G8P
//   splitk M N K          -> slices tiles_per_slice tiles_in_last_slice workspace_bytes
//   tn M N K lddy ldx     -> TN256|TN128 slices pairs_per_slice
// Pointers are only tested by the route, never dereferenced: a fixed 4096-aligned address stands in.
#include <cstdio>
#include <cstring>

#include "../../vimo_clip_amd/csrc/gemm_route.h"

int main() {
  char kind[16];
  void* const base = (void*)(uintptr_t)0x10000;
  static const char* fam[] = {"TILE", "G8", "G8P"};
  while (scanf("%15s", kind) == 1) {
    if (!strcmp(kind, "linear")) {
      int M, N, K, lda, ldw, ldc, ldres, ldz, act, bias, res, Z, od, rd, org, rrm, dt, variant, cfg, ks, u, m32;
      if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &M, &N, &K, &lda, &ldw, &ldc, &ldres, &ldz, &act, &bias,
                &res, &Z, &od, &rd, &org, &rrm, &dt, &variant, &cfg, &ks, &u, &m32) != 22)
        return 2;
      const GemmProblem p{base, base, bias ? base : nullptr, res ? base : nullptr, base, Z ? base : nullptr, M, N, K, lda, ldw, ldc, ldres, ldz,
                          act, 1.0f, od, rd, org, rrm, dt};
      GemmOverrides ov;
      ov.cfg = cfg; ov.ks = ks != 0; ov.u = u; ov.mfma32 = m32 != 0;
      if (const int rc = gemm_check(p, variant)) {
        printf("rc %d\n", rc);
        continue;
      }
      const GemmPlan pl = gemm_route(p, variant, ov);
      printf("%d", pl.n);
      for (int i = 0; i < pl.n; ++i) printf(" %s %d %d %d", fam[pl.launch[i].family], pl.launch[i].cfg, pl.launch[i].row0, pl.launch[i].rows);
      printf("\n");
    } else if (!strcmp(kind, "splitk")) {
      int M, N, K;
      if (scanf("%d %d %d", &M, &N, &K) != 3) return 2;
      const int s = splitk_slices(M, N, K), nkt = K / 64, per = (nkt + s - 1) / s;
      printf("%d %d %d %zu\n", s, per, nkt - (s - 1) * per, splitk_workspace_bytes(M, N, K));
    } else if (!strcmp(kind, "tn")) {
      int M, N, K, lddy, ldx;
      if (scanf("%d %d %d %d %d", &M, &N, &K, &lddy, &ldx) != 5) return 2;
      const TnPlan t = tn_route(M, N, K, lddy, ldx, GemmOverrides());
      printf("%s %d %d\n", t.k256 ? "TN256" : "TN128", t.slices, t.pairs_per_slice);
    } else {
      return 2;
    }
  }
  return 0;
}
