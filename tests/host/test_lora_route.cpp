// Host test of vimo_clip_amd/csrc/lora_route.h: the argument checks of vmc_lora_down_concat / vmc_lora_wgrad_tn, the down kernel's plan
// (rank tiles, rows per workgroup, K chunk, LDS) over a sweep of shapes, the weight-gradient plan (column tiles, token slices, workspace)
// with every token covered exactly once, and the plans of the shapes the towers and the GPU tests issue.  Built with g++ by
// tests/test_host_lora_route.py.
#include <cstdio>
#include <initializer_list>

#include "../../vimo_clip_amd/csrc/lora_route.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

int main() {
  const uintptr_t P = 0x10000;      // an aligned address
  // ---- vmc_lora_down_concat: checks ----------------------------------------------------------------------------------------------
  CHECK(lora_check_down(P, P, P, 768, 768, 832, 25600, 768, 16, 768) == 0, "the B/32 in_proj call refused");
  CHECK(lora_check_down(P, P, P, 776, 776, 840, 1, 768, 8, 776) == 0, "M = 1, padded leading dimensions, col0 > K refused");
  CHECK(lora_check_down(0, P, P, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ARG, "NULL x");
  CHECK(lora_check_down(P, 0, P, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ARG, "NULL a16");
  CHECK(lora_check_down(P, P, 0, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ARG, "NULL out");
  for (int r : {0, 4, 12, 72, -8}) CHECK(lora_check_down(P, P, P, 768, 768, 832, 8, 768, r, 768) == VMC_E_SHAPE, "r = %d accepted", r);
  for (int K : {0, 32, 96, 800}) CHECK(lora_check_down(P, P, P, 4096, 4096, 4096, 8, K, 16, 1024) == VMC_E_SHAPE, "K = %d accepted", K);
  CHECK(lora_check_down(P, P, P, 768, 768, 832, 0, 768, 16, 768) == VMC_E_SHAPE, "M = 0");
  CHECK(lora_check_down(P, P, P, 768, 768, 832, 8, 768, 16, 760) == VMC_E_SHAPE, "col0 < K");
  CHECK(lora_check_down(P, P, P, 768, 768, 840, 8, 768, 16, 772) == VMC_E_SHAPE, "col0 % 8");
  CHECK(lora_check_down(P, P, P, 768, 768, 824, 8, 768, 16, 768) == VMC_E_SHAPE, "ldo < col0 + 64");
  CHECK(lora_check_down(P, P, P, 760, 768, 832, 8, 768, 16, 768) == VMC_E_SHAPE, "ldx < K");
  CHECK(lora_check_down(P, P, P, 768, 704, 832, 8, 768, 16, 768) == VMC_E_SHAPE, "lda < K");
  CHECK(lora_check_down(P + 2, P, P, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ALIGN, "x + 2 bytes");
  CHECK(lora_check_down(P, P + 8, P, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ALIGN, "a16 + 8 bytes");
  CHECK(lora_check_down(P, P, P + 4, 768, 768, 832, 8, 768, 16, 768) == VMC_E_ALIGN, "out + 4 bytes");
  CHECK(lora_check_down(P, P, P, 772, 768, 832, 8, 768, 16, 768) == VMC_E_ALIGN, "ldx % 8");
  CHECK(lora_check_down(P, P, P, 768, 770, 832, 8, 768, 16, 768) == VMC_E_ALIGN, "lda % 8");
  CHECK(lora_check_down(P, P, P, 768, 768, 836, 8, 768, 16, 768) == VMC_E_ALIGN, "ldo % 8");
  // ---- vmc_lora_down_concat: plans -----------------------------------------------------------------------------------------------
  for (int r = 8; r <= 64; r += 8)
    for (int K = 64; K <= 4096; K += 64)
      for (int M : {1, 15, 16, 63, 64, 65, 136, 1000, 25600, 65535, 65536, 65792, 131072, 1 << 20}) {
        ++cases;
        const LoraDownPlan p = lora_route_down(M, K, r);
        CHECK(p.rc == 0, "M%d K%d r%d refused", M, K, r);
        CHECK(p.nt >= 1 && p.nt <= 4 && 16 * p.nt >= r && 16 * (p.nt - 1) < r, "nt %d for r %d", p.nt, r);
        CHECK((p.rt == 1 || p.rt == LORA_DOWN_MAX_RT) && p.rows_per_wg == LORA_DOWN_ROWS * p.rt, "rt %d", p.rt);
        CHECK((long long)p.grid * p.rows_per_wg >= M && (long long)(p.grid - 1) * p.rows_per_wg < M, "M%d: grid %u x %d rows", M, p.grid, p.rows_per_wg);
        CHECK(p.rt == 1 || p.grid >= 2u * LORA_CUS, "M%d: two row tiles per wave with %u workgroups", M, p.grid);
        CHECK(p.kc % 64 == 0 && p.kc >= 64 && p.kc <= K && p.kc <= 512 && (p.kc == K || p.kc >= 256), "K%d r%d: kc %d", K, r, p.kc);
        CHECK(p.lds == 16 * p.nt * (p.kc + 8) * 2 && p.lds <= 40 * 1024, "K%d r%d: LDS %d", K, r, p.lds);      // four workgroups per CU
      }
  CHECK(lora_route_down(8, 96, 16).rc == VMC_E_SHAPE && lora_route_down(8, 128, 12).rc == VMC_E_SHAPE && lora_route_down(0, 128, 16).rc == VMC_E_SHAPE,
        "a bad shape planned");
  {  // the towers at r = 16: ViT-B/32 at 512 frames (25 600 rows), ViT-L/14 at 256 frames (65 792 rows)
    const LoraDownPlan b = lora_route_down(25600, 768, 16), bp = lora_route_down(25600, 3072, 16), l = lora_route_down(65792, 1024, 16);
    CHECK(b.nt == 1 && b.rt == 1 && b.kc == 512 && b.grid == 400, "B/32 in_proj: nt %d rt %d kc %d grid %u", b.nt, b.rt, b.kc, b.grid);
    CHECK(bp.kc == 512 && bp.grid == 400 && bp.lds == 16 * 520 * 2, "B/32 c_proj: kc %d grid %u lds %d", bp.kc, bp.grid, bp.lds);
    CHECK(l.rt == 2 && l.grid == 514, "L/14 in_proj: rt %d grid %u", l.rt, l.grid);
    const LoraDownPlan w = lora_route_down(136, 4096, 64);      // the widest rank at the deepest K (tests/lora_refs.py)
    CHECK(w.nt == 4 && w.kc == 256 && w.grid == 3 && w.lds == 64 * 264 * 2, "r64: nt %d kc %d grid %u lds %d", w.nt, w.kc, w.grid, w.lds);
  }
  // ---- vmc_lora_wgrad_tn ---------------------------------------------------------------------------------------------------------
  for (int r = 8; r <= 64; r += 8)
    for (int C : {8, 64, 128, 136, 520, 768, 1024, 2304, 3072, 4096})
      for (int M : {1, 63, 64, 65, 255, 256, 257, 1100, 2500, 25600, 65792, 1 << 20}) {
        ++cases;
        const LoraWgradPlan p = lora_route_wgrad(M, r, C);
        CHECK(p.rc == 0, "M%d r%d C%d refused", M, r, C);
        CHECK(p.nt == (r + 15) / 16 && p.c_tiles == (C + LORA_WG_COLS - 1) / LORA_WG_COLS, "tiles");
        CHECK(p.slices >= 1 && p.slices <= LORA_WG_MAX_SLICES && p.tokens_per_slice % LORA_WG_TOKENS == 0, "M%d C%d: %d slices of %d", M, C, p.slices, p.tokens_per_slice);
        // every token in exactly one slice, no empty slice
        CHECK((long long)p.slices * p.tokens_per_slice >= M && (long long)(p.slices - 1) * p.tokens_per_slice < M, "M%d C%d: %d x %d", M, C, p.slices, p.tokens_per_slice);
        CHECK(p.slices == 1 || 2 * p.tokens_per_slice >= LORA_WG_MIN_SLICE, "M%d C%d: %d slices of only %d tokens", M, C, p.slices, p.tokens_per_slice);
        CHECK(p.workspace_bytes == (p.slices > 1 ? (size_t)p.slices * r * C * 4 : 0), "workspace");
        CHECK(M < 2 * LORA_CUS * LORA_WG_MIN_SLICE || p.slices * p.c_tiles >= LORA_CUS, "M%d C%d: %d workgroups", M, C, p.slices * p.c_tiles);
        CHECK(lora_check_wgrad(P, P, P, 64, C, M, r, C, P, p.workspace_bytes) == 0, "M%d r%d C%d: call refused", M, r, C);
        if (p.workspace_bytes) {
          CHECK(lora_check_wgrad(P, P, P, 64, C, M, r, C, P, p.workspace_bytes - 1) == VMC_E_ARG, "short workspace accepted");
          CHECK(lora_check_wgrad(P, P, P, 64, C, M, r, C, 0, p.workspace_bytes) == VMC_E_ARG, "NULL workspace accepted");
          CHECK(lora_check_wgrad(P, P, P, 64, C, M, r, C, P + 8, p.workspace_bytes) == VMC_E_ALIGN, "misaligned workspace accepted");
        }
      }
  {  // the cases of tests/lora_refs.py and the towers
    const LoraWgradPlan a = lora_route_wgrad(65, 64, 64), b = lora_route_wgrad(1100, 16, 136), c = lora_route_wgrad(2500, 8, 520);
    CHECK(a.slices == 1 && a.tokens_per_slice == 128 && a.workspace_bytes == 0 && a.nt == 4, "65 x 64 x 64: %d x %d", a.slices, a.tokens_per_slice);
    CHECK(b.slices == 5 && b.tokens_per_slice == 256 && b.c_tiles == 2 && b.nt == 1, "1100 x 16 x 136: %d x %d", b.slices, b.tokens_per_slice);
    CHECK(c.slices == 10 && c.tokens_per_slice == 256 && c.c_tiles == 5 && c.nt == 1, "2500 x 8 x 520: %d x %d", c.slices, c.tokens_per_slice);
    const LoraWgradPlan t = lora_route_wgrad(25600, 16, 768);
    CHECK(t.c_tiles == 6 && t.slices == 80 && t.tokens_per_slice == 320, "B/32 dA: %d tiles, %d x %d", t.c_tiles, t.slices, t.tokens_per_slice);
  }
  CHECK(lora_check_wgrad(0, P, P, 64, 64, 8, 16, 64, 0, 0) == VMC_E_ARG && lora_check_wgrad(P, P, 0, 64, 64, 8, 16, 64, 0, 0) == VMC_E_ARG, "NULL operand");
  for (int r : {0, 4, 12, 72}) CHECK(lora_check_wgrad(P, P, P, 128, 64, 8, r, 64, 0, 0) == VMC_E_SHAPE, "r = %d accepted", r);
  CHECK(lora_check_wgrad(P, P, P, 64, 68, 8, 16, 60, 0, 0) == VMC_E_SHAPE && lora_check_wgrad(P, P, P, 64, 64, 0, 16, 64, 0, 0) == VMC_E_SHAPE, "C % 8 / M = 0");
  CHECK(lora_check_wgrad(P, P, P, 8, 64, 8, 16, 64, 0, 0) == VMC_E_SHAPE && lora_check_wgrad(P, P, P, 64, 56, 8, 16, 64, 0, 0) == VMC_E_SHAPE, "ldt < r / ldx < C");
  CHECK(lora_check_wgrad(P + 2, P, P, 64, 64, 8, 16, 64, 0, 0) == VMC_E_ALIGN && lora_check_wgrad(P, P, P, 68, 64, 8, 16, 64, 0, 0) == VMC_E_ALIGN, "alignment");
  printf("%d shapes, %d failures\n", cases, fails);
  if (!fails) printf("OK\n");
  return fails ? 1 : 0;
}
