// Host test of the fused TFAM chain dispatch (vimo_clip_amd/csrc/tfam_route.h): the launches of whole calls for the shapes of
// tfam_route_recorded.h, every exit of tfam_check, a soundness sweep over the product of the decision classes (a shape that
// tfam_check accepts plans every launch of its chain, each an instantiated kernel inside its launch bounds, 160 KB of LDS, the
// K-slice exchange area and the weight-gradient table; every instantiated kernel is planned by some shape), and the workspace sizes.
// The expected plans were recorded from the chains as they dispatched before the routing moved into tfam_route.h (a host-side print
// in front of every launch, checked against a GPU kernel trace), so a change of routing shows up here instead of only as a different
// time, or an exception, on the GPU.  Built with g++ by tests/test_host_tfam_route.py.
//
// A launch reads "<kernel>:grid:block:dynamic LDS bytes":
//   S<BN>.<PRO>.<EPI>.<KD>.<DH>.<QT>.<NKT>.<TR> tf_gemm_kernel      P<BN>.<PRO>.<EPI>.<KD>.<TR> tf_gemm_pair_kernel
//   R<BN>.<KC>.<TR> tf_gemm_ring_kernel      O<D> tf_pool_kernel      H1.<MAXB> H2.<MAXB> H3.<D> tr_head_bwd{1,2,3}_kernel
//   G<problems>.<LayerNorm problems> tr_wgrad_group_kernel
// A call is its launches in order: eval = vmc_tfam_forward; train = vmc_tfam_train_fwd, then vmc_tfam_train_bwd (the two
// vmc_attention_bwd calls per layer are attn_route.h's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../vimo_clip_amd/csrc/tfam_route.h"
#include "tfam_route_recorded.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static bool inst_seen[kTfamInstCount];

static std::string dims_str(const TfDims& d, bool train) {
  char b[160];
  snprintf(b, sizeof b, "%s B%d T%d Tk%d D%d H%d ff%d L%d C%d cross%d", train ? "train" : "eval", d.B, d.T, d.Tk, d.D, d.H, d.ff, d.L, d.C, d.has_cross);
  return b;
}

static std::string plan_str(const TfamPlan& p, int nprob = 0, int nln = 0) {
  if (p.rc) return "err=" + std::to_string(p.rc);
  char k[64], b[128];
  switch (p.family) {
    case TFAM_SINGLE: snprintf(k, sizeof k, "S%d.%d.%d.%d.%d.%d.%d.%d", p.bn, p.pro, p.epi, p.kd, p.dh, p.qt, p.nkt, p.tr); break;
    case TFAM_PAIR: snprintf(k, sizeof k, "P%d.%d.%d.%d.%d", p.bn, p.pro, p.epi, p.kd, p.tr); break;
    case TFAM_RING: snprintf(k, sizeof k, "R%d.%d.%d", p.bn, p.kc, p.tr); break;
    case TFAM_POOL: snprintf(k, sizeof k, "O%d", p.kd); break;
    case TFAM_HEAD_BWD1: snprintf(k, sizeof k, "H1.%d", p.maxb); break;
    case TFAM_HEAD_BWD2: snprintf(k, sizeof k, "H2.%d", p.maxb); break;
    case TFAM_HEAD_BWD3: snprintf(k, sizeof k, "H3.%d", p.kd); break;
    case TFAM_WGRAD: snprintf(k, sizeof k, "G%d.%d", nprob, nln); break;
    default: snprintf(k, sizeof k, "family%d", p.family);
  }
  snprintf(b, sizeof b, "%s:%u:%d:%d", k, p.grid, p.block, p.lds);
  return b;
}

// a planned launch names an instantiated kernel and stays inside its __launch_bounds__, 160 KB of dynamic LDS, a 31-bit grid, and
// (single-shot kernels) the A image that the K-slice exchange reuses
static void check_plan(const std::string& name, const TfamPlan& p) {
  CHECK(p.rc == 0, "%s: rc %d", name.c_str(), p.rc);
  if (p.rc || p.family == TFAM_NONE) return;
  const int i = tfam_find_inst(p);
  CHECK(i >= 0, "%s: no instantiated kernel for %s", name.c_str(), plan_str(p).c_str());
  if (i < 0) return;
  inst_seen[i] = true;
  CHECK(p.block >= 64 && p.block % 64 == 0 && p.block <= kTfamInsts[i].bound, "%s: %s: launch bound %d", name.c_str(), plan_str(p).c_str(), kTfamInsts[i].bound);
  CHECK(p.lds >= 0 && (size_t)p.lds <= TF_LDS_MAX, "%s: %s: LDS", name.c_str(), plan_str(p).c_str());
  CHECK(p.grid > 0 && p.grid <= 0x7FFFFFFFu, "%s: %s: grid", name.c_str(), plan_str(p).c_str());
  if (p.family == TFAM_SINGLE) {
    CHECK((TF_NW / 2 - 1) * 2 * (p.bn / 16) * 1024 <= TF_BM * p.kd * 2, "%s: %s: K-slice exchange", name.c_str(), plan_str(p).c_str());
    CHECK(p.grid == (unsigned)(p.n_tiles * p.n_rb), "%s: %s: grid != tiles x row blocks", name.c_str(), plan_str(p).c_str());
  }
  if (p.family == TFAM_PAIR) CHECK(p.grid == (unsigned)(p.n_tiles * p.n_rb + p.n_tiles_b * p.n_rb_b), "%s: %s: pair grid", name.c_str(), plan_str(p).c_str());
}

template <int N>
static void add_step(std::string& out, const std::string& name, const TfamStep<N>& s, bool check) {
  for (int i = 0; i < N; ++i) {
    if (check) check_plan(name, s.p[i]);
    if (s.p[i].rc || s.p[i].family != TFAM_NONE) out += (out.empty() ? "" : " ") + plan_str(s.p[i]);
  }
}

// the launches of one whole call
static std::string chain(const TfDims& d, bool train, const TfamOverrides& ov, bool check) {
  const std::string name = dims_str(d, train);
  const TfamBlocks b = tfam_blocks(d);
  std::string out;
  for (int l = 0; l < d.L; ++l) add_step(out, name, tfam_route_layer_fwd(d, b, l == 0, true, train, ov), check);
  add_step(out, name, tfam_route_head_fwd(d, train, ov), check);
  if (!train) {
    if (check) {      // the per-layer entries: vmc_tfam_layer_fwd without the pair, vmc_tfam_kv_fwd
      std::string unused;
      for (int first = 0; first < 2; ++first) add_step(unused, name, tfam_route_layer_fwd(d, b, first, false, false, ov), true);
      if (d.has_cross) check_plan(name, tfam_route_kv(d, b, ov));
    }
    return out;
  }
  add_step(out, name, tfam_route_head_bwd(d), check);
  const TfamWgradLayer w = tfam_wgrad_layer(d);
  for (int l = d.L - 1; l >= 0; --l) {
    add_step(out, name, tfam_route_layer_bwd(d, b, l == 0, ov), check);
    if (const int n = tfam_wgrad_flush(d.L, l)) {
      const TfamPlan g = tfam_route_wgrad(d, n);
      if (check) {
        check_plan(name, g);
        CHECK(n <= TR_WGRAD_FLUSH && n * w.nprob <= TR_MAX_PROB && n * w.nln <= TR_MAX_LN, "%s: %d layers in one weight-gradient launch", name.c_str(), n);
      }
      out += " " + plan_str(g, n * w.nprob, n * w.nln);
    } else if (check) {
      CHECK(l > 0, "%s: no weight-gradient launch after layer 0", name.c_str());
    }
  }
  if (check) check_plan(name, tfam_route_wgrad(d, 1));      // vmc_tfam_layer_bwd launches its own layer's
  return out;
}

static void test_recorded() {
  bool seen_T[3] = {}, seen_Tk[3] = {}, seen_flush = false, seen_env = false, seen_b40 = false;
  for (const Recorded& r : kRecorded) {
    ++cases;
    const TfDims d = {r.B, r.T, r.Tk, r.D, r.H, r.ff, r.L, r.C, r.cross};
    TfamOverrides ov;
    ov.bn_ff = r.bn_ff;
    ov.bn_d = r.bn_d;
    const std::string name = dims_str(d, r.train) + (r.bn_ff ? " switches " + std::to_string(r.bn_ff) : "");
    const int rc = tfam_check(d, r.train);
    if (r.state == 0) {
      CHECK(rc == 0, "%s: ran before, now refused (%d)", name.c_str(), rc);
      const std::string got = chain(d, r.train, ov, false);
      CHECK(got == r.plans, "%s:\n  got      %s\n  recorded %s", name.c_str(), got.c_str(), r.plans);
      if (r.train) {
        CHECK(tfam_train_workspace_bytes(d) == r.ws, "%s: training workspace %zu, recorded %llu", name.c_str(), tfam_train_workspace_bytes(d), r.ws);
        CHECK(tfam_train_pool_grad_offset(d) == r.pool_off, "%s: pool gradient offset", name.c_str());
      }
      seen_T[r.T <= 16 ? 0 : r.T <= 32 ? 1 : 2] = true;
      if (r.cross) seen_Tk[r.Tk <= 16 ? 0 : r.Tk <= 32 ? 1 : 2] = true;
      seen_flush |= r.train && r.L == 5;
      seen_env |= r.bn_ff != 0;
      seen_b40 |= !r.train && r.B == 40;
    } else {
      // failed mid-chain before, or was declined by the Python gate (its conditions are tfam_check's now): refused up front
      CHECK(rc == VMC_E_SHAPE, "%s: state %d before, tfam_check now %d", name.c_str(), r.state, rc);
    }
    if (!r.train) {
      TfDims e = d;
      e.H = 8;      // vmc_tfam_workspace_bytes does not take the head count
      CHECK(tfam_workspace_bytes(e) == r.ws, "%s: workspace %zu, recorded %llu", name.c_str(), tfam_workspace_bytes(e), r.ws);
    }
  }
  CHECK(seen_T[0] && seen_T[1] && seen_T[2] && seen_Tk[0] && seen_Tk[1] && seen_Tk[2] && seen_flush && seen_env && seen_b40, "recorded list lost a decision class");
}

// every exit of tfam_check: each tuple breaks exactly one condition of a shape that is otherwise taken
static void test_check_exits() {
  const TfDims ok = {8, 16, 16, 768, 8, 2048, 4, 140, 1};
  CHECK(tfam_check(ok, false) == 0 && tfam_check(ok, true) == 0, "the reference geometry is refused");
  struct Exit { const char* what; TfDims d; int eval_rc, train_rc; };
  const int E = VMC_E_SHAPE;
  const Exit exits[] = {
      {"B = 0", {0, 16, 16, 768, 8, 2048, 4, 140, 1}, E, E},
      {"T = 0", {8, 0, 16, 768, 8, 2048, 4, 140, 1}, E, E},
      {"T = 65", {2, 65, 16, 768, 8, 2048, 4, 140, 1}, E, E},
      {"L = 0", {8, 16, 16, 768, 8, 2048, 0, 140, 1}, E, E},
      {"C = 0", {8, 16, 16, 768, 8, 2048, 4, 0, 1}, E, E},
      {"D = 640", {8, 16, 16, 640, 10, 2048, 4, 140, 1}, E, E},
      {"H = 0", {8, 16, 16, 768, 0, 2048, 4, 140, 1}, E, E},
      {"H = 7 does not divide D", {8, 16, 16, 768, 7, 2048, 4, 140, 1}, E, E},
      {"head dim 128", {8, 16, 16, 768, 6, 2048, 4, 140, 1}, E, E},
      {"head dim 32", {8, 16, 16, 512, 16, 2048, 4, 140, 1}, E, E},
      {"ff = 0", {8, 16, 16, 768, 8, 0, 4, 140, 1}, E, E},
      {"ff = 1000", {8, 16, 16, 768, 8, 1000, 4, 140, 1}, E, E},
      {"Tk = 0 with cross attention", {8, 16, 0, 768, 8, 2048, 4, 140, 1}, E, E},
      {"Tk = 65", {2, 16, 65, 768, 8, 2048, 4, 140, 1}, E, E},
      {"Tk = 0 without cross attention", {8, 16, 0, 768, 8, 2048, 4, 140, 0}, 0, 0},
      {"B T = 272 rows", {17, 16, 16, 768, 8, 2048, 4, 140, 1}, 0, E},
      {"B Tk = 264 motion rows", {8, 16, 33, 512, 8, 2048, 4, 140, 1}, 0, E},
      {"B = 33", {33, 4, 4, 768, 8, 2048, 4, 140, 1}, 0, E},
      {"C = 141", {8, 16, 16, 768, 8, 2048, 4, 141, 1}, 0, E},
      {"C = 480", {2, 16, 16, 512, 8, 2048, 4, 480, 1}, 0, 0},
      {"C = 484: the head backward's dlogits rows leave its LDS", {2, 16, 16, 512, 8, 2048, 4, 484, 1}, 0, E},
      // two clips' keys per row block beside the W tile: refused up front (these failed after launches had been issued)
      {"T = 16, Tk = 26, D = 768", {2, 16, 26, 768, 8, 2048, 4, 140, 1}, 0, 0},
      {"T = 16, Tk = 27, D = 768", {2, 16, 27, 768, 8, 2048, 4, 140, 1}, E, E},
      {"T = 16, Tk = 64, D = 768", {2, 16, 64, 768, 8, 2048, 4, 140, 1}, E, E},
      {"T = 17, Tk = 64, D = 768", {2, 17, 64, 768, 8, 2048, 4, 140, 1}, 0, 0},
      {"T = 16, Tk = 63, D = 512", {2, 16, 63, 512, 8, 2048, 4, 140, 1}, 0, 0},
      {"T = 16, Tk = 64, D = 512", {2, 16, 64, 512, 8, 2048, 4, 140, 1}, E, E},
  };
  for (const Exit& e : exits) {
    ++cases;
    CHECK(tfam_check(e.d, false) == e.eval_rc, "%s: eval %d, expected %d", e.what, tfam_check(e.d, false), e.eval_rc);
    CHECK(tfam_check(e.d, true) == e.train_rc, "%s: train %d, expected %d", e.what, tfam_check(e.d, true), e.train_rc);
  }
}

static void test_sweep() {
  const int Ts[] = {1, 16, 17, 32, 33, 64}, DH[][2] = {{512, 8}, {768, 8}, {768, 12}}, ffs[] = {512, 1024, 2048};
  const int Bs[] = {1, 2, 8, 9, 16, 32, 40}, Cs[] = {4, 140, 480, 484}, Ls[] = {1, 4, 5}, sw[] = {0, 16, 32, 48, 64};
  long accepted = 0, refused = 0;
  for (int T : Ts) for (int Tk : Ts) for (auto& dh : DH) for (int ff : ffs) for (int B : Bs) for (int C : Cs) for (int cross = 0; cross < 2; ++cross)
    for (int L : Ls) for (int train = 0; train < 2; ++train) for (int s : sw) {
      if (s && !train) continue;      // the switches are the training chain's
      const TfDims d = {B, T, cross ? Tk : 0, dh[0], dh[1], ff, L, C, cross};
      if (!cross && Tk != Ts[0]) continue;
      TfamOverrides ov;
      ov.bn_ff = ov.bn_d = s;
      if (tfam_check(d, train)) { ++refused; continue; }
      ++accepted;
      chain(d, train, ov, true);
    }
  cases += (int)(accepted + refused);
  CHECK(accepted > 1000 && refused > 1000, "sweep: %ld accepted, %ld refused", accepted, refused);
  for (int i = 0; i < kTfamInstCount; ++i) {
    const TfamInst& k = kTfamInsts[i];
    CHECK(inst_seen[i], "kTfamInsts[%d] (family %d bn %d pro %d epi %d kd %d dh %d qt %d nkt %d tr %d kc %d maxb %d) is planned by no shape", i, k.family, k.bn,
          k.pro, k.epi, k.kd, k.dh, k.qt, k.nkt, k.tr, k.kc, k.maxb);
  }
}

template <typename W>
static void check_aligned(const char* what, const W& w, size_t npointers) {
  uintptr_t p[64];
  memcpy(p, &w, npointers * sizeof(uintptr_t));
  for (size_t i = 0; i < npointers; ++i) CHECK(p[i] % 256 == 0, "%s: sub-buffer %zu at offset %zu", what, i, (size_t)p[i]);
}

static void test_workspaces() {
  for (int train = 0; train < 2; ++train) {
    size_t prev_T = 0;
    for (int T = 1; T <= 64; ++T) {
      size_t prev_B = 0;
      for (int B = 1; B <= (train ? 256 / T < 32 ? 256 / T : 32 : 40); ++B) {
        ++cases;
        const TfDims d = {B, T, T, 768, 8, 2048, 4, 140, 1};
        const size_t n = train ? tfam_train_workspace_bytes(d) : tfam_workspace_bytes(d);
        CHECK(n % 256 == 0 && n > prev_B, "workspace not growing with B at B %d T %d train %d", B, T, train);
        prev_B = n;
        if (B == 1) {
          CHECK(n >= prev_T, "workspace shrinking with T at T %d train %d", T, train);
          prev_T = n;
        }
        if (train) {
          const TrWs w = tr_ws(nullptr, d);
          check_aligned("TrWs", w, 11);
          CHECK(w.layer_bytes % 256 == 0, "layer stride");
          check_aligned("TrLayerWs", tr_lw(w, d, d.L - 1), sizeof(TrLayerWs) / sizeof(void*));
        } else {
          check_aligned("TfWs", tf_ws(nullptr, d), 12);
        }
      }
    }
  }
}

int main() {
  test_recorded();
  test_check_exits();
  test_sweep();
  test_workspaces();
  if (fails) {
    printf("%d checks failed over %d cases\n", fails, cases);
    return 1;
  }
  printf("OK %d cases\n", cases);
  return 0;
}
