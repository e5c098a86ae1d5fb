// Host test of the input-gradient section of vimo_clip_amd/csrc/tfam_route.h (gradients wrt the tokens of the training chains): a sweep
// over d_model x heads x clip length x batch x depth x (no cross attention | cross attention | projection).  Every shape that the chain
// itself accepts is accepted by tfam_check_input; its plans name kernels of kTfamInputInsts and stay inside TF_LDS_MAX; the
// extension starts at the end of the workspace it extends, is 256-byte aligned, and its pieces do not overlap; the sizes and
// offsets of the existing workspaces are what they were.  Built with g++ by tests/test_host_tfam_input_route.py.
#include <cstdio>
#include <initializer_list>

#include "../../vimo_clip_amd/csrc/tfam_route.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static bool inst_seen[kTfamInputInstCount];

static void plan_ok(const TfamPlan& p, const char* what, int D, int T, int B) {
  CHECK(p.rc == 0, "%s D%d T%d B%d: rc %d", what, D, T, B, p.rc);
  const int i = tfam_find_input_inst(p);
  CHECK(i >= 0, "%s D%d T%d B%d: names no kernel of kTfamInputInsts", what, D, T, B);
  if (i >= 0) {
    inst_seen[i] = true;
    CHECK(p.block == kTfamInputInsts[i].bound, "%s block %d", what, p.block);
  }
  CHECK(p.lds > 0 && (size_t)p.lds <= TF_LDS_MAX, "%s D%d: LDS %d", what, D, p.lds);
  CHECK(p.grid == (unsigned)(p.n_tiles * p.n_rb) && p.grid > 0, "%s grid", what);
}

int main() {
  int accepted[3] = {0, 0, 0};
  for (int D : {512, 768})
    for (int H : {8, 12})
      for (int T = 1; T <= 64; ++T)
        for (int B = 1; B * T <= 256 && B <= 40; ++B)
          for (int L : {1, 2, 4, 8})
            for (int mode = 0; mode < 3; ++mode) {      // 0: one stream, 1: cross attention, 2: projection
              const int ff = L == 1 ? 512 : 2048, C = 140, Tk = mode == 1 ? (T > 1 ? T - 1 : 1) : 0;
              TfDims d = {B, T, Tk, D, H, ff, L, C, mode == 1, mode == 2};
              ++cases;
              const int rc_chain = mode == 2 ? tfam_check_proj(d) : tfam_check(d, true);
              const int rc = tfam_check_input(d);
              CHECK(rc == rc_chain, "D%d H%d T%d B%d L%d mode %d: input check %d, chain %d", D, H, T, B, L, mode, rc, rc_chain);
              if (rc) continue;
              ++accepted[mode];
              const TfamBlocks b = tfam_blocks(d);
              const size_t M = (size_t)B * T, Mk = (size_t)B * Tk;
              const TrInputWs iw = tr_input_ws(nullptr, d);
              if (mode == 2) {
                const TfamPlan p = tfam_route_input_dxcat(d);
                plan_ok(p, "dXcat", D, T, B);
                CHECK(p.family == TFAM_SINGLE && p.bn == 16 && p.pro == PRO_16 && p.epi == EPI_BIAS32 && p.kd == D && p.tr == 1, "dXcat fields");
                CHECK(p.n_tiles * 16 == 2 * D && p.n_rb * TF_BM >= (int)M && (p.n_rb - 1) * TF_BM < (int)M, "dXcat tiles %d x %d", p.n_tiles, p.n_rb);
                CHECK(p.lds == (TF_BM + 16) * D * 2, "dXcat LDS %d", p.lds);
                CHECK((TF_NW / 2 - 1) * 2 * (p.bn / 16) * 1024 <= TF_BM * p.kd * 2, "dXcat K-slice exchange");
                // the extension lies behind the projection's, whose layout is unchanged
                const TrProjWs pw = tr_proj_ws(nullptr, d);
                CHECK((uintptr_t)iw.dxcat == pw.bytes && pw.bytes == tfam_train_proj_workspace_bytes(d), "dXcat does not start at the end of the projection workspace");
                CHECK(iw.bytes >= pw.bytes + M * 2 * D * 4 && iw.bytes % 256 == 0 && (uintptr_t)iw.dxcat % 256 == 0, "dXcat extent");
                CHECK(iw.dx == nullptr && iw.dmotion == nullptr, "projection mode has no dX / dMotion");
                TfDims plain = d;
                plain.proj = 0;
                CHECK(tfam_train_workspace_bytes(d) == tfam_train_workspace_bytes(plain), "training workspace size changed");
                CHECK((uintptr_t)pw.x32 == tfam_train_workspace_bytes(plain) && tfam_train_proj_dx0_offset(d) == (long long)(uintptr_t)pw.dx0, "projection offsets changed");
              } else {
                const TfamPlan px = tfam_route_input_dx(d, b);
                plan_ok(px, "dX", D, T, B);
                CHECK(px.family == TFAM_RING && (3 * D) % px.kc == 0 && px.grid == (unsigned)((D / TF_RING_BN) * b.n_rb), "dX ring kc %d grid %u", px.kc, px.grid);
                if (L > 1) {
                  const TfamPlan l8 = tfam_route_layer_bwd(d, b, false, TfamOverrides()).p[TFAM_B_DX0];
                  CHECK(l8.grid == px.grid && l8.kc == px.kc && l8.lds == px.lds, "dX differs from L8 of the other layers");
                }
                CHECK(tfam_route_layer_bwd(d, b, true, TfamOverrides()).p[TFAM_B_DX0].family == TFAM_NONE, "the plain chain's layer 0 has no L8");
                const TfamPlan pm = tfam_route_input_dmotion(d, b);
                if (mode == 1) {
                  plan_ok(pm, "dMotion", D, T, B);
                  CHECK(pm.family == TFAM_RING && pm.kc == TF_RING_KC && (2 * D) % pm.kc == 0, "dMotion ring kc %d", pm.kc);
                  CHECK(pm.n_tiles * TF_RING_BN == D && pm.n_rb * TF_BM >= (int)Mk && (pm.n_rb - 1) * TF_BM < (int)Mk, "dMotion tiles %d x %d", pm.n_tiles, pm.n_rb);
                } else {
                  CHECK(pm.rc == 0 && pm.family == TFAM_NONE, "dMotion planned without cross attention");
                }
                const TrWs w = tr_ws(nullptr, d);
                CHECK(w.bytes == tfam_train_workspace_bytes(d) && (uintptr_t)iw.dx == w.bytes, "dX does not start at the end of the training workspace");
                CHECK((uintptr_t)iw.dx % 256 == 0 && iw.bytes % 256 == 0 && iw.dxcat == nullptr, "dX alignment");
                if (mode == 1) {
                  CHECK((uintptr_t)iw.dmotion >= (uintptr_t)iw.dx + M * D * 4 && (uintptr_t)iw.dmotion % 256 == 0, "dMotion overlaps dX");
                  CHECK(iw.bytes >= (uintptr_t)iw.dmotion + Mk * D * 4, "dMotion extent");
                } else {
                  CHECK(iw.dmotion == nullptr && iw.bytes >= (uintptr_t)iw.dx + M * D * 4, "dX extent");
                }
                CHECK(tfam_train_pool_grad_offset(d) == (long long)(uintptr_t)tr_lw(w, d, L - 1).dx3, "pool gradient offset changed");
              }
              CHECK(tfam_train_input_workspace_bytes(d) == iw.bytes, "extension size");
            }
  for (int i = 0; i < kTfamInputInstCount; ++i) {
    const TfamInst& k = kTfamInputInsts[i];
    // the KC = 384 ring serves dX at d_model 768 (K = 2304); everything else is reached by some shape as well
    CHECK(inst_seen[i], "kTfamInputInsts[%d] (family %d, K %d, KC %d) is reached by no shape", i, k.family, k.kd, k.kc);
  }
  CHECK(accepted[0] > 1000 && accepted[1] > 1000 && accepted[2] > 1000, "sweep too thin: %d %d %d", accepted[0], accepted[1], accepted[2]);
  {  // recorded sizes of the existing workspaces at the reference shapes: unchanged by this section
    TfDims cross = {8, 16, 15, 512, 8, 2048, 4, 140, 1}, proj = {8, 15, 0, 768, 8, 2048, 4, 140, 0, 1};
    const size_t al = 255;
    CHECK(tfam_train_input_workspace_bytes(cross) == tfam_train_workspace_bytes(cross) + ((128 * 512 * 4 + al) & ~al) + ((120 * 512 * 4 + al) & ~al), "cross extension size");
    CHECK(tfam_train_input_workspace_bytes(proj) == tfam_train_proj_workspace_bytes(proj) + ((120 * 1536 * 4 + al) & ~al), "projection extension size");
    TfDims bad = cross;
    bad.B = 17;
    CHECK(tfam_check_input(bad) == VMC_E_SHAPE, "more than 256 rows accepted");
    TfDims pc = proj;
    pc.has_cross = 1; pc.Tk = 15;
    CHECK(tfam_check_input(pc) == VMC_E_SHAPE, "projection with cross attention accepted");
  }
  printf("%d shapes, accepted %d / %d / %d, %d failures\n", cases, accepted[0], accepted[1], accepted[2], fails);
  if (!fails) printf("OK\n");
  return fails ? 1 : 0;
}
