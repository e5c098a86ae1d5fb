// Host test of the feature-concatenation section of vimo_clip_amd/csrc/tfam_route.h (projection_layer in front of layer 0 of the
// training chains): a sweep over d_model x clip length x batch x depth.  Every shape that tfam_check_proj accepts plans F0, layer 0's
// qkv dgrad and the weight-gradient group with the projection's problem; every entry of kTfamProjInsts is reached; F0 stays inside
// TF_LDS_MAX; the workspace extension is 256-byte aligned and leaves every offset of the training workspace where it is without a
// projection.  Built with g++ by tests/test_host_tfam_proj_route.py.
#include <cstdio>
#include <initializer_list>

#include "../../vimo_clip_amd/csrc/tfam_route.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static bool inst_seen[kTfamProjInstCount];

int main() {
  const TfamOverrides ov;
  int accepted = 0, refused_depth = 0;
  for (int D : {512, 768})
    for (int H : {8, 12})
      for (int T = 1; T <= 64; ++T)
        for (int B = 1; B * T <= 256 && B <= 40; ++B)
          for (int L : {1, 2, 4, 8}) {
            const int ff = L == 1 ? 512 : 2048, C = 140;
            TfDims d = {B, T, 0, D, H, ff, L, C, 0, 1};
            TfDims plain = {B, T, 0, D, H, ff, L, C, 0};
            ++cases;
            const int rc = tfam_check_proj(d), rc_plain = tfam_check(plain, true);
            if (rc_plain) CHECK(rc != 0, "D%d H%d T%d B%d L%d: accepted, but the training chain refuses the shape", D, H, T, B, L);
            if (L * tfam_wgrad_layer(d).nprob + 1 > TR_MAX_PROB) {
              CHECK(rc == VMC_E_SHAPE, "D%d T%d B%d L%d: %d problems accepted", D, T, B, L, L * tfam_wgrad_layer(d).nprob + 1);
              if (!rc_plain) ++refused_depth;
            }
            if (rc) continue;
            ++accepted;
            CHECK(rc_plain == 0 && L * 4 + 1 <= TR_MAX_PROB, "D%d T%d B%d L%d", D, T, B, L);
            const TfamBlocks b = tfam_blocks(d);
            // F0
            const TfamPlan f0 = tfam_route_proj_fwd(d);
            CHECK(f0.rc == 0, "D%d T%d B%d L%d: F0 rc %d", D, T, B, L, f0.rc);
            const int i = tfam_find_proj_inst(f0);
            CHECK(i >= 0, "D%d T%d B%d: F0 names no instantiated kernel", D, T, B);
            CHECK(tfam_find_inst(f0) < 0, "F0's kernel is also in kTfamInsts");
            if (i >= 0) {
              inst_seen[i] = true;
              CHECK(f0.block == kTfamProjInsts[i].bound, "F0 block %d", f0.block);
            }
            CHECK(f0.kd == 2 * D && f0.bn == 16 && f0.pro == PRO_F32 && f0.epi == EPI_BIAS32 && f0.tr == 1, "F0 fields");
            CHECK(f0.lds > 0 && (size_t)f0.lds <= TF_LDS_MAX && f0.lds == (TF_BM + 16) * 2 * D * 2, "F0 LDS %d", f0.lds);
            CHECK((TF_NW / 2 - 1) * 2 * (f0.bn / 16) * 1024 <= TF_BM * f0.kd * 2, "F0 K-slice exchange");
            CHECK(f0.n_tiles * 16 == D && f0.n_rb * TF_BM >= b.M && (f0.n_rb - 1) * TF_BM < b.M, "F0 tiles %d x %d", f0.n_tiles, f0.n_rb);
            CHECK(f0.grid == (unsigned)(f0.n_tiles * f0.n_rb) && f0.grid > 0, "F0 grid");
            // L8 of layer 0: the ring the other layers run
            const TfamPlan l8 = tfam_route_proj_bwd(d, b);
            CHECK(l8.rc == 0 && l8.family == TFAM_RING && tfam_find_inst(l8) >= 0, "D%d T%d B%d: L8(0) rc %d", D, T, B, l8.rc);
            CHECK((3 * D) % l8.kc == 0 && (size_t)l8.lds <= TF_LDS_MAX && l8.block == TF_NTH, "L8(0) kc %d lds %d", l8.kc, l8.lds);
            CHECK(l8.grid == (unsigned)((D / TF_RING_BN) * b.n_rb), "L8(0) grid %u", l8.grid);
            if (L > 1) {
              const TfamStep<TFAM_B_COUNT> sb = tfam_route_layer_bwd(d, b, false, ov);
              CHECK(sb.p[TFAM_B_DX0].grid == l8.grid && sb.p[TFAM_B_DX0].kc == l8.kc && sb.p[TFAM_B_DX0].lds == l8.lds, "L8(0) differs from L8(l > 0)");
            }
            CHECK(tfam_route_layer_bwd(d, b, true, ov).p[TFAM_B_DX0].family == TFAM_NONE, "the plain chain's layer 0 has no L8");
            // the grouped launch that holds layer 0's problems: the one-call backward's last flush and the per-layer entry's own
            const int pending = tfam_wgrad_flush(L, 0);
            CHECK(pending >= 1 && pending <= TR_WGRAD_FLUSH, "flush after layer 0: %d", pending);
            for (int n : {pending, 1}) {
              const TfamPlan g = tfam_route_proj_wgrad(d, n), g0 = tfam_route_wgrad(d, n);
              CHECK(g.rc == 0 && g0.rc == 0 && g.family == TFAM_WGRAD && tfam_find_inst(g) >= 0, "wgrad rc %d", g.rc);
              CHECK(n * tfam_wgrad_layer(d).nprob + 1 <= TR_MAX_PROB && n * tfam_wgrad_layer(d).nln <= TR_MAX_LN, "wgrad table");
              CHECK(g.grid == g0.grid + (unsigned)(((D + 255) / 256) * (2 * D / 128)), "wgrad grid %u vs %u", g.grid, g0.grid);
              CHECK(g.block == TR_WGRAD_NTH && g.lds == TR_WGRAD_LDS, "wgrad launch");
            }
            // workspace: the extension sits behind the training workspace, which keeps its size and offsets
            const TrWs w0 = tr_ws(nullptr, plain), w1 = tr_ws(nullptr, d);
            CHECK(tfam_train_workspace_bytes(d) == tfam_train_workspace_bytes(plain) && w0.bytes == w1.bytes, "training workspace size changed");
            CHECK(tfam_train_pool_grad_offset(d) == tfam_train_pool_grad_offset(plain), "pool gradient offset changed");
            CHECK(w0.layer_bytes == w1.layer_bytes && w0.layers == w1.layers && w0.dpl == w1.dpl, "training workspace layout changed");
            const TrProjWs pw = tr_proj_ws(nullptr, d);
            const size_t M = (size_t)B * T;
            const uintptr_t o[5] = {(uintptr_t)pw.x32, (uintptr_t)pw.xcat16, (uintptr_t)pw.dx0, (uintptr_t)pw.d0_16, (uintptr_t)pw.bytes};
            const size_t need[4] = {M * D * 4, M * 2 * D * 2, M * D * 4, M * D * 2};
            CHECK(o[0] == w0.bytes, "the extension does not start at the end of the training workspace");
            for (int k = 0; k < 4; ++k) {
              CHECK(o[k] % 256 == 0, "extension buffer %d at %zu: not 256-byte aligned", k, (size_t)o[k]);
              CHECK(o[k + 1] >= o[k] + need[k], "extension buffer %d overlaps the next", k);
            }
            CHECK(pw.bytes % 256 == 0 && tfam_train_proj_workspace_bytes(d) == pw.bytes, "extension size");
            CHECK(tfam_train_proj_dx0_offset(d) == (long long)o[2], "dx0 offset");
          }
  for (int i = 0; i < kTfamProjInstCount; ++i) CHECK(inst_seen[i], "kTfamProjInsts[%d] (K = %d) is reached by no shape", i, kTfamProjInsts[i].kd);
  CHECK(accepted > 1000 && refused_depth > 100, "sweep too thin: %d accepted, %d refused for depth", accepted, refused_depth);
  {  // exits of tfam_check_proj
    TfDims ok = {4, 15, 0, 512, 8, 2048, 4, 140, 0, 1};
    CHECK(tfam_check_proj(ok) == 0, "reference shape refused");
    TfDims l7 = ok, l8 = ok, cross = ok, rows = ok, cls = ok;
    l7.L = 7; l8.L = 8; cross.has_cross = 1; cross.Tk = 16; rows.B = 18; cls.C = 141;
    CHECK(tfam_check_proj(l7) == 0, "7 layers (29 problems) refused");
    CHECK(tfam_check_proj(l8) == VMC_E_SHAPE, "8 layers (33 problems) accepted");
    CHECK(tfam_check_proj(cross) == VMC_E_SHAPE, "cross attention accepted");
    CHECK(tfam_check_proj(rows) == VMC_E_SHAPE && tfam_check_proj(cls) == VMC_E_SHAPE, "a shape outside the training set accepted");
    CHECK(tfam_route_proj_wgrad(l8, 8).rc == VMC_E_SHAPE, "33 problems planned");
  }
  printf("%d shapes, %d accepted, %d refused for depth, %d failures\n", cases, accepted, refused_depth, fails);
  if (!fails) printf("OK\n");
  return fails ? 1 : 0;
}
