// Host test of the attention dispatch (vimo_clip_amd/csrc/attn_route.h): the plans for the shapes the models and the GPU tests
// issue, every VMC_ATTN_VARIANT class, the LDS-fit and alignment fallbacks, every error exit in the order the arguments are
// checked, and that every plan names an instantiated kernel inside its launch bounds.  The expected plans were recorded from the
// dispatch as it stood before it moved into attn_route.h, so a change of routing shows up here instead of only as a different
// time on the GPU.  Built with g++ by tests/test_host_attn_route.py.
//
// A plan reads "kernel g=grid0/grid1/grid2 b=block lds=dynamic LDS bytes rs=row stride st=stagger", an error "err=<VMC code>".
// vit<NT,NC,NW,REREAD,PERSIST> = attn_vit_kernel, vl<NC> / vlc<NC> = attn_vit_long_kernel / attn_vit_long_cls_kernel,
// small<DH,NT> = attn_small_kernel, long_fwd<DH>, long_bwd<DH> (delta, dK / dV, dQ grids) = attention_long.hip, bwd_mfma<DH> =
// attn_bwd_mfma_kernel, generic_fwd / generic_bwd (dQ, dK / dV grids) = the scalar kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../vimo_clip_amd/csrc/attn_route.h"

static int fails = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static bool vit_seen[kAttnVitInstCount], inst_seen[kAttnInstCount];

static std::string plan_str(const AttnPlan& p) {
  if (p.rc) return "err=" + std::to_string(p.rc);
  char k[64], b[192];
  if (p.kernel == ATTN_VIT && p.vit >= 0 && p.vit < kAttnVitInstCount) {
    const AttnVitInst& c = kAttnVitInsts[p.vit];
    snprintf(k, sizeof k, "vit<%d,%d,%d,%d,%d>", c.nt, c.nc, c.nw, (int)c.reread, (int)c.persist);
  } else if (p.kernel == ATTN_VIT_LONG) snprintf(k, sizeof k, "vl<%d>", p.nc);
  else if (p.kernel == ATTN_VIT_LONG_CLS) snprintf(k, sizeof k, "vlc<%d>", p.nc);
  else if (p.kernel == ATTN_SMALL) snprintf(k, sizeof k, "small<%d,%d>", p.dh, p.nt);
  else if (p.kernel == ATTN_LONG_FWD) snprintf(k, sizeof k, "long_fwd<%d>", p.dh);
  else if (p.kernel == ATTN_GENERIC_FWD) snprintf(k, sizeof k, "generic_fwd");
  else if (p.kernel == ATTN_BWD_MFMA) snprintf(k, sizeof k, "bwd_mfma<%d>", p.dh);
  else if (p.kernel == ATTN_LONG_BWD) snprintf(k, sizeof k, "long_bwd<%d>", p.dh);
  else if (p.kernel == ATTN_GENERIC_BWD) snprintf(k, sizeof k, "generic_bwd");
  else snprintf(k, sizeof k, "kernel%d/%d", p.kernel, p.vit);
  snprintf(b, sizeof b, "%s g=%u/%u/%u b=%d lds=%d rs=%d st=%d", k, p.grid[0], p.grid[1], p.grid[2], p.block, p.lds, p.rs, p.stagger);
  return b;
}

// every launch names an instantiated kernel and stays inside its __launch_bounds__, 160 KB of dynamic LDS and 31-bit grids
static void check_plan(const char* name, const AttnPlan& p) {
  if (p.rc) return;
  int bound = 0;
  if (p.kernel == ATTN_VIT) {
    CHECK(p.vit >= 0 && p.vit < kAttnVitInstCount && p.dh == 0 && p.nt == 0 && p.nc == 0, "%s: vit entry %d", name, p.vit);
    if (p.vit >= 0 && p.vit < kAttnVitInstCount) {
      bound = 64 * kAttnVitInsts[p.vit].nw;
      vit_seen[p.vit] = true;
      CHECK(p.lds == 16 * kAttnVitInsts[p.vit].nt * 128 * 2, "%s: LDS %d for %d key tiles", name, p.lds, kAttnVitInsts[p.vit].nt);
    }
  } else {
    for (int i = 0; i < kAttnInstCount; ++i) {
      const AttnInst& k = kAttnInsts[i];
      if (k.kernel == p.kernel && k.dh == p.dh && k.nt == p.nt && k.nc == p.nc) {
        bound = k.bound;
        inst_seen[i] = true;
      }
    }
  }
  CHECK(bound > 0, "%s: no instantiated kernel for %s", name, plan_str(p).c_str());
  CHECK(p.block >= 64 && p.block % 64 == 0 && p.block <= bound, "%s: %d threads, launch bound %d", name, p.block, bound);
  CHECK(p.lds >= 0 && p.lds <= ATT_BWD_MAX_LDS, "%s: %d bytes of dynamic LDS", name, p.lds);
  const int ngrids = p.kernel == ATTN_LONG_BWD ? 3 : p.kernel == ATTN_GENERIC_BWD ? 2 : 1;
  for (int i = 0; i < 3; ++i)
    CHECK(i < ngrids ? p.grid[i] > 0 && p.grid[i] <= 0x7FFFFFFFu : p.grid[i] == 0, "%s: grid[%d] = %u", name, i, p.grid[i]);
  CHECK(p.kernel == ATTN_BWD_MFMA ? p.rs == 2 * p.dh || p.rs == 2 * p.dh + 16 : p.rs == 0, "%s: row stride %d", name, p.rs);
  CHECK(p.kernel == ATTN_VIT || p.stagger == 0, "%s: stagger %d", name, p.stagger);
}

static void want(const char* name, const AttnPlan& p, const char* expect) {
  ++cases;
  const std::string got = plan_str(p);
  CHECK(got == expect, "%s: %s, want %s", name, got.c_str(), expect);
  check_plan(name, p);
}

static const void* cp(uintptr_t a) { return (const void*)a; }
static void* wp(uintptr_t a) { return (void*)a; }

// the operands vmc_attention_vit_fwd builds from the packed qkv, or (cls) vmc_attention_vit_cls_fwd from q_cls and the packed kv
static AttnVitProblem vit(int F, int N, int H, bool cls, int dt = VMC_BF16) {
  const size_t D = (size_t)H * 64;
  if (cls) return {cp(0x100000), cp(0x4000000), cp(0x4000000 + 2 * D), wp(0x8000000), nullptr, D, 2 * D, F, N, 1, H, dt};
  return {cp(0x100000), cp(0x100000 + 2 * D), cp(0x100000 + 4 * D), wp(0x8000000), (float*)0x9000000, 3 * D, 3 * D, F, N, N, H, dt};
}
// TFAM self attention (q | k | v packed, stride 3D) or cross attention (q stride D, k | v packed, stride 2D); out stride D
static AttnFwdProblem fwd(int B, int H, int Tq, int Tk, int dh, bool cross = false) {
  const int D = H * dh, ldkv = cross ? 2 * D : 3 * D;
  return {cp(0x100000), cp(0x200000), cp(0x300000), nullptr, wp(0x400000), nullptr, B, H, Tq, Tk, dh, cross ? D : 3 * D, ldkv, ldkv, D,
          0.f, 0, VMC_BF16};
}
// q, out, dout, dq stride D; k | v and dk | dv packed, stride 2D; the workspace as vmc_attention_bwd_workspace_bytes sizes it
static AttnBwdProblem bwd(int B, int H, int Tq, int Tk, int dh) {
  const int D = H * dh;
  return {cp(0x100000), cp(0x200000), cp(0x300000), nullptr, cp(0x400000), cp(0x500000), (const float*)0x600000, wp(0x700000),
          wp(0x800000), wp(0x900000), B, H, Tq, Tk, dh, D, 2 * D, 2 * D, D, D, 2 * D, 2 * D, 0.f, 0, wp(0xA00000),
          attn_bwd_workspace_bytes(B, H, Tq), VMC_BF16};
}

struct VitCase { int F, N, H; bool cls; int variant; const char* want; };
static const VitCase kVitCases[] = {
    {2, 5, 16, false, 1, "vit<2,0,4,0,0> g=32/0/0 b=256 lds=8192 rs=0 st=0"},
    {2, 17, 16, false, 1, "vit<2,0,4,0,0> g=32/0/0 b=256 lds=8192 rs=0 st=0"},
    {2, 32, 16, false, 1, "vit<2,0,4,0,0> g=32/0/0 b=256 lds=8192 rs=0 st=0"},
    {2, 33, 16, false, 1, "vit<4,0,4,0,0> g=32/0/0 b=256 lds=16384 rs=0 st=0"},
    {2, 50, 16, false, 1, "vit<4,50,4,0,0> g=32/0/0 b=256 lds=16384 rs=0 st=0"},
    {2, 64, 16, false, 1, "vit<4,0,4,0,0> g=32/0/0 b=256 lds=16384 rs=0 st=0"},
    {2, 65, 16, false, 1, "vit<8,0,4,0,0> g=32/0/0 b=256 lds=32768 rs=0 st=0"},
    {2, 128, 16, false, 1, "vit<8,0,4,0,0> g=32/0/0 b=256 lds=32768 rs=0 st=0"},
    {2, 129, 16, false, 1, "vit<14,0,4,0,0> g=32/0/0 b=256 lds=57344 rs=0 st=0"},
    {2, 197, 16, false, 1, "vit<14,197,4,0,0> g=32/0/0 b=256 lds=57344 rs=0 st=0"},
    {2, 224, 16, false, 1, "vit<14,0,4,0,0> g=32/0/0 b=256 lds=57344 rs=0 st=0"},
    {2, 225, 16, false, 1, "vit<18,0,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 256, 16, false, 1, "vit<18,0,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 1, "vit<18,257,8,1,0> g=32/0/0 b=512 lds=73728 rs=0 st=0"},
    {2, 258, 16, false, 1, "vit<18,0,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 288, 16, false, 1, "vit<18,0,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 289, 16, false, 1, "vl<0> g=96/0/0 b=256 lds=0 rs=0 st=0"},
    {2, 577, 16, false, 1, "vl<577> g=160/0/0 b=256 lds=0 rs=0 st=0"},
    {2, 1025, 16, false, 1, "vl<0> g=288/0/0 b=256 lds=0 rs=0 st=0"},
    {3, 577, 5, false, 1, "vl<577> g=75/0/0 b=256 lds=0 rs=0 st=0"},
    {256, 577, 16, false, 1, "vl<577> g=20480/0/0 b=256 lds=0 rs=0 st=0"},
    // the class query (the last encoder block)
    {2, 5, 16, true, 1, "vit<2,0,4,0,0> g=32/0/0 b=256 lds=8192 rs=0 st=0"},
    {2, 17, 16, true, 1, "vit<2,0,4,0,0> g=32/0/0 b=256 lds=8192 rs=0 st=0"},
    {2, 50, 16, true, 1, "vit<4,50,4,0,0> g=32/0/0 b=256 lds=16384 rs=0 st=0"},
    {2, 197, 16, true, 1, "vit<14,197,4,0,0> g=32/0/0 b=256 lds=57344 rs=0 st=0"},
    {2, 257, 16, true, 1, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 288, 16, true, 1, "vit<18,0,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 289, 16, true, 1, "vlc<0> g=8/0/0 b=256 lds=131072 rs=0 st=0"},
    {2, 577, 16, true, 1, "vlc<577> g=8/0/0 b=256 lds=131072 rs=0 st=0"},
    {2, 1025, 16, true, 1, "vlc<0> g=8/0/0 b=256 lds=131072 rs=0 st=0"},
    {3, 577, 5, true, 1, "vlc<577> g=4/0/0 b=256 lds=131072 rs=0 st=0"},
    // VMC_ATTN_VARIANT at N = 257: only the full call follows it
    {2, 257, 16, false, 2, "vit<18,257,4,1,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 9, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 0, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 10, "vit<18,257,4,0,1> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 12, "vit<18,257,4,0,1> g=32/0/0 b=256 lds=73728 rs=0 st=2"},
    {2, 257, 16, false, 19, "vit<18,257,4,0,1> g=32/0/0 b=256 lds=73728 rs=0 st=9"},
    {2, 257, 16, false, 20, "vit<18,257,8,1,1> g=32/0/0 b=512 lds=73728 rs=0 st=0"},
    {2, 257, 16, false, 21, "vit<18,257,8,1,1> g=32/0/0 b=512 lds=73728 rs=0 st=1"},
    {2, 257, 16, false, 29, "vit<18,257,8,1,1> g=32/0/0 b=512 lds=73728 rs=0 st=9"},
    {2, 257, 16, false, 30, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {64, 257, 16, false, 1, "vit<18,257,8,1,0> g=1024/0/0 b=512 lds=73728 rs=0 st=0"},
    {64, 257, 16, false, 12, "vit<18,257,4,0,1> g=512/0/0 b=256 lds=73728 rs=0 st=2"},
    {64, 257, 16, false, 21, "vit<18,257,8,1,1> g=512/0/0 b=512 lds=73728 rs=0 st=1"},
    {2, 257, 16, true, 2, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, true, 12, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 257, 16, true, 21, "vit<18,257,4,0,0> g=32/0/0 b=256 lds=73728 rs=0 st=0"},
    {2, 197, 16, false, 2, "vit<14,197,4,0,0> g=32/0/0 b=256 lds=57344 rs=0 st=0"},
    {2, 577, 16, false, 2, "vl<577> g=160/0/0 b=256 lds=0 rs=0 st=0"},
};

struct FwdCase { int B, H, Tq, Tk, dh; bool cross; const char* want; };
static const FwdCase kFwdCases[] = {
    // TFAM self / cross attention of one clip
    {8, 8, 16, 16, 64, false, "small<64,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 32, 32, 64, false, "small<64,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 40, 40, 64, false, "small<64,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 64, 64, 64, false, "small<64,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 16, 16, 96, false, "small<96,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 32, 32, 96, false, "small<96,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 40, 40, 96, false, "small<96,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 64, 64, 96, false, "small<96,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 16, 16, 64, true, "small<64,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 32, 32, 64, true, "small<64,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 40, 40, 64, true, "small<64,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 64, 64, 64, true, "small<64,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 16, 16, 96, true, "small<96,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 32, 32, 96, true, "small<96,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 40, 40, 96, true, "small<96,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 64, 64, 96, true, "small<96,4> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    {4, 8, 16, 15, 96, true, "small<96,2> g=32/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 65, 16, 64, true, "small<64,2> g=64/0/0 b=64 lds=0 rs=0 st=0"},
    // the per-op path of whole videos: the tiled kernel
    {8, 8, 65, 65, 64, false, "long_fwd<64> g=128/0/0 b=256 lds=0 rs=0 st=0"},
    {8, 8, 65, 65, 96, true, "long_fwd<96> g=128/0/0 b=256 lds=0 rs=0 st=0"},
    {8, 8, 16, 65, 64, true, "long_fwd<64> g=64/0/0 b=256 lds=0 rs=0 st=0"},
    {2, 2, 100, 257, 64, true, "long_fwd<64> g=8/0/0 b=256 lds=0 rs=0 st=0"},
    {8, 8, 2199, 2199, 64, false, "long_fwd<64> g=2240/0/0 b=256 lds=0 rs=0 st=0"},
    {8, 8, 2199, 2199, 96, true, "long_fwd<96> g=2240/0/0 b=256 lds=0 rs=0 st=0"},
    // other head dims: the scalar kernel, Tq, Tk <= 2048
    {8, 8, 16, 16, 32, false, "generic_fwd g=1024/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 2048, 2048, 32, false, "generic_fwd g=131072/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 2048, 2048, 128, true, "generic_fwd g=131072/0/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 2049, 16, 32, false, "err=-3"},
    {8, 8, 16, 2049, 128, true, "err=-3"},
};

struct BwdCase { int B, H, Tq, Tk, dh; const char* want; };
static const BwdCase kBwdCases[] = {
    // whole head in LDS: one wave per tile task (at most 4), rows padded by 16 B while that fits
    {8, 8, 16, 16, 64, "bwd_mfma<64> g=64/0/0 b=128 lds=18688 rs=144 st=0"},
    {8, 8, 16, 16, 96, "bwd_mfma<96> g=64/0/0 b=128 lds=26880 rs=208 st=0"},
    {4, 8, 16, 15, 96, "bwd_mfma<96> g=32/0/0 b=128 lds=26880 rs=208 st=0"},
    {8, 8, 16, 32, 64, "bwd_mfma<64> g=64/0/0 b=192 lds=18688 rs=144 st=0"},
    {8, 8, 32, 32, 64, "bwd_mfma<64> g=64/0/0 b=256 lds=18688 rs=144 st=0"},
    {8, 8, 40, 40, 64, "bwd_mfma<64> g=64/0/0 b=256 lds=37376 rs=144 st=0"},
    {8, 8, 64, 64, 96, "bwd_mfma<96> g=64/0/0 b=256 lds=53760 rs=208 st=0"},
    {8, 8, 65, 65, 64, "bwd_mfma<64> g=64/0/0 b=256 lds=56064 rs=144 st=0"},
    {8, 12, 50, 50, 64, "bwd_mfma<64> g=96/0/0 b=256 lds=37376 rs=144 st=0"},          // ViT-B/32
    {8, 8, 256, 256, 64, "bwd_mfma<64> g=64/0/0 b=256 lds=149504 rs=144 st=0"},
    {2, 16, 257, 257, 64, "bwd_mfma<64> g=32/0/0 b=256 lds=149760 rs=128 st=0"},        // the student at N = 257: unpadded rows
    {8, 8, 288, 288, 64, "bwd_mfma<64> g=64/0/0 b=256 lds=149760 rs=128 st=0"},
    {8, 8, 192, 192, 96, "bwd_mfma<96> g=64/0/0 b=256 lds=161280 rs=208 st=0"},
    // past the LDS: the tiled passes
    {8, 8, 289, 289, 64, "long_bwd<64> g=289/320/320 b=256 lds=0 rs=0 st=0"},
    {8, 8, 193, 193, 96, "long_bwd<96> g=193/256/256 b=256 lds=0 rs=0 st=0"},
    {8, 8, 2199, 2199, 96, "long_bwd<96> g=2199/2240/2240 b=256 lds=0 rs=0 st=0"},
    // other head dims: the scalar kernels
    {8, 8, 16, 16, 32, "generic_bwd g=1024/1024/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 2048, 2048, 128, "generic_bwd g=131072/131072/0 b=64 lds=0 rs=0 st=0"},
    {8, 8, 2049, 16, 128, "err=-3"},
    {8, 8, 16, 2049, 32, "err=-3"},
};

int main() {
  char name[160];
  for (const VitCase& c : kVitCases)
    for (int dt : {VMC_BF16, VMC_F16}) {
      AttnOverrides ov;
      ov.variant = c.variant;
      snprintf(name, sizeof name, "vit%s F=%d N=%d H=%d variant=%d dtype=%d", c.cls ? " cls" : "", c.F, c.N, c.H, c.variant, dt);
      want(name, attn_vit_route(vit(c.F, c.N, c.H, c.cls, dt), ov), c.want);
    }
  for (const FwdCase& c : kFwdCases)
    for (int dt : {VMC_BF16, VMC_F16}) {
      AttnFwdProblem p = fwd(c.B, c.H, c.Tq, c.Tk, c.dh, c.cross);
      p.dtype16 = dt;
      snprintf(name, sizeof name, "fwd B=%d H=%d Tq=%d Tk=%d dh=%d%s dtype=%d", c.B, c.H, c.Tq, c.Tk, c.dh, c.cross ? " cross" : "", dt);
      want(name, attn_fwd_route(p), c.want);
      p.dropout_p = 0.25f;                                        // dropout does not change the route
      want(name, attn_fwd_route(p), c.want);
    }
  for (const BwdCase& c : kBwdCases)
    for (int dt : {VMC_BF16, VMC_F16}) {
      AttnBwdProblem p = bwd(c.B, c.H, c.Tq, c.Tk, c.dh);
      p.dtype16 = dt;
      snprintf(name, sizeof name, "bwd B=%d H=%d Tq=%d Tk=%d dh=%d dtype=%d", c.B, c.H, c.Tq, c.Tk, c.dh, dt);
      want(name, attn_bwd_route(p), c.want);
    }

  // alignment fallbacks: the tiled forward stores out as 8-byte words; attn_small_kernel does too, within ldo % 8 == 0 rows
  AttnFwdProblem f = fwd(8, 8, 65, 65, 64);
  f.out = wp(0x400004);
  want("fwd out & 7, Tk = 65", attn_fwd_route(f), "generic_fwd g=4160/0/0 b=64 lds=0 rs=0 st=0");
  f.out = wp(0x400008);
  want("fwd out 8-byte aligned, Tk = 65", attn_fwd_route(f), "long_fwd<64> g=128/0/0 b=256 lds=0 rs=0 st=0");
  f = fwd(8, 8, 64, 64, 64);
  f.out = wp(0x400004);
  want("fwd out & 7, Tk = 64", attn_fwd_route(f), "small<64,4> g=64/0/0 b=64 lds=0 rs=0 st=0");
  f = fwd(8, 8, 2199, 2199, 96);
  f.out = wp(0x400002);
  want("fwd out & 7, Tk = 2199", attn_fwd_route(f), "err=-3");
  f = fwd(8, 8, 65, 65, 64);
  f.ldo = 514;                                                    // ldo % 4 != 0 never reaches a kernel: ldo % 8 is checked first
  want("fwd ldo = 514", attn_fwd_route(f), "err=-2");
  f.ldo = 516;
  want("fwd ldo = 516", attn_fwd_route(f), "err=-2");
  // ... the tiled backward stores dq, dk, dv as 8-byte words and reads out as 16-byte words; the in-LDS kernel needs neither
  AttnBwdProblem b = bwd(8, 8, 289, 289, 64);
  b.dq = wp(0x700004);
  want("bwd dq & 7, T = 289", attn_bwd_route(b), "generic_bwd g=18496/18496/0 b=64 lds=0 rs=0 st=0");
  b = bwd(8, 8, 289, 289, 64);
  b.dk = wp(0x800002);
  want("bwd dk & 7, T = 289", attn_bwd_route(b), "generic_bwd g=18496/18496/0 b=64 lds=0 rs=0 st=0");
  b = bwd(8, 8, 289, 289, 64);
  b.dv = wp(0x900006);
  want("bwd dv & 7, T = 289", attn_bwd_route(b), "generic_bwd g=18496/18496/0 b=64 lds=0 rs=0 st=0");
  b = bwd(8, 8, 289, 289, 64);
  b.out = cp(0x400008);
  want("bwd out & 15, T = 289", attn_bwd_route(b), "generic_bwd g=18496/18496/0 b=64 lds=0 rs=0 st=0");
  b = bwd(8, 8, 289, 289, 64);
  b.dq = wp(0x700008);
  want("bwd dq 8-byte aligned, T = 289", attn_bwd_route(b), "long_bwd<64> g=289/320/320 b=256 lds=0 rs=0 st=0");
  b = bwd(8, 8, 16, 16, 64);
  b.dq = wp(0x700004);
  b.out = cp(0x400008);
  want("bwd dq & 7, out & 15, T = 16", attn_bwd_route(b), "bwd_mfma<64> g=64/0/0 b=128 lds=18688 rs=144 st=0");
  b = bwd(8, 8, 16, 16, 64);
  b.lddq = 514;
  want("bwd lddq % 4, T = 16", attn_bwd_route(b), "generic_bwd g=1024/1024/0 b=64 lds=0 rs=0 st=0");
  b = bwd(8, 8, 2199, 2199, 96);
  b.dq = wp(0x700004);
  want("bwd dq & 7, T = 2199", attn_bwd_route(b), "err=-3");

  // every error exit, one bad argument at a time, and which of two wins (the order the arguments are checked in)
  struct VitErr { const char* what; int want; void (*bad)(AttnVitProblem&); };
  static const VitErr kVitErr[] = {
      {"q=0", VMC_E_ARG, [](AttnVitProblem& p) { p.q = nullptr; }},
      {"k=0", VMC_E_ARG, [](AttnVitProblem& p) { p.k = nullptr; }},
      {"out=0", VMC_E_ARG, [](AttnVitProblem& p) { p.out = nullptr; }},
      {"F=0", VMC_E_ARG, [](AttnVitProblem& p) { p.F = 0; }},
      {"N=0", VMC_E_ARG, [](AttnVitProblem& p) { p.N = 0; }},
      {"N=-1", VMC_E_ARG, [](AttnVitProblem& p) { p.N = -1; }},
      {"H=0", VMC_E_ARG, [](AttnVitProblem& p) { p.H = 0; }},
      {"q+8", VMC_E_ALIGN, [](AttnVitProblem& p) { p.q = cp(0x100008); }},
      {"k+8", VMC_E_ALIGN, [](AttnVitProblem& p) { p.k = cp((uintptr_t)p.k + 8); }},
      {"out+4", VMC_E_ALIGN, [](AttnVitProblem& p) { p.out = wp(0x8000004); }},
      {"dtype=0", VMC_E_DTYPE, [](AttnVitProblem& p) { p.dtype16 = 0; }},
      {"dtype=3", VMC_E_DTYPE, [](AttnVitProblem& p) { p.dtype16 = 3; }},
      {"dtype=3 N=577", VMC_E_DTYPE, [](AttnVitProblem& p) { p.dtype16 = 3; p.N = p.NQ = 577; }},
      {"N=0 dtype=0", VMC_E_ARG, [](AttnVitProblem& p) { p.N = 0; p.dtype16 = 0; }},
      {"q+8 dtype=0", VMC_E_ALIGN, [](AttnVitProblem& p) { p.q = cp(0x100008); p.dtype16 = 0; }},
      {"out=0 q+8", VMC_E_ARG, [](AttnVitProblem& p) { p.out = nullptr; p.q = cp(0x100008); }},
      {"N=577 grid > 2^31", VMC_E_SHAPE, [](AttnVitProblem& p) { p.N = p.NQ = 577; p.F = 1 << 20; p.H = 1 << 10; }},
      {"N=577 grid > 2^31 dtype=0", VMC_E_DTYPE, [](AttnVitProblem& p) { p.N = p.NQ = 577; p.F = 1 << 20; p.H = 1 << 10; p.dtype16 = 0; }},
      {"cls N=577 F*H > 2^31", VMC_E_SHAPE, [](AttnVitProblem& p) { p.N = 577; p.NQ = 1; p.F = 1 << 16; p.H = 1 << 15; }},
      {"cls N=577 F*H = 2^31 - 2^16", 0, [](AttnVitProblem& p) { p.N = 577; p.NQ = 1; p.F = 1 << 16; p.H = (1 << 15) - 1; }},
      {"(valid)", 0, [](AttnVitProblem& p) { (void)p; }},
  };
  for (const VitErr& c : kVitErr) {
    AttnVitProblem p = vit(2, 50, 16, false);
    c.bad(p);
    const int rc = attn_vit_route(p, AttnOverrides()).rc;
    CHECK(rc == c.want, "vit %s: %d, want %d", c.what, rc, c.want);
    ++cases;
  }

  struct FwdErr { const char* what; int want; void (*bad)(AttnFwdProblem&); };
  static const FwdErr kFwdErr[] = {      // on the TFAM self-attention shape B = H = 8, T = 64, dh 64 (attn_small_kernel)
      {"q=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.q = nullptr; }},
      {"k=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.k = nullptr; }},
      {"v=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.v = nullptr; }},
      {"out=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.out = nullptr; }},
      {"dropout=-0.5", VMC_E_ARG, [](AttnFwdProblem& p) { p.dropout_p = -0.5f; }},
      {"dropout=1", VMC_E_ARG, [](AttnFwdProblem& p) { p.dropout_p = 1.0f; }},
      {"B=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.B = 0; }},
      {"H=-1", VMC_E_ARG, [](AttnFwdProblem& p) { p.H = -1; }},
      {"Tq=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.Tq = 0; }},
      {"Tk=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.Tk = 0; }},
      {"dh=0", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.dh = 0; }},
      {"dh=60", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.dh = 60; }},
      {"dh=136", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.dh = 136; }},
      {"ldq=1540", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.ldq = 1540; }},
      {"ldk=1540", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.ldk = 1540; }},
      {"ldv=1540", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.ldv = 1540; }},
      {"ldo=516", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.ldo = 516; }},
      {"q+8", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.q = cp(0x100008); }},
      {"k+8", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.k = cp(0x200008); }},
      {"v+2", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.v = cp(0x300002); }},
      {"dtype=0 (small)", VMC_E_DTYPE, [](AttnFwdProblem& p) { p.dtype16 = 0; }},
      {"dtype=3 Tk=65 (tiled)", VMC_E_DTYPE, [](AttnFwdProblem& p) { p.dtype16 = 3; p.Tq = p.Tk = 65; }},
      {"dtype=0 dh=32 (scalar)", VMC_E_DTYPE, [](AttnFwdProblem& p) { p.dtype16 = 0; p.dh = 32; }},
      {"dtype=0 dh=32 Tq=2049", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.dtype16 = 0; p.dh = 32; p.Tq = 2049; }},
      {"tiled grid > 2^31", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.B = 1 << 20; p.H = 64; p.Tq = p.Tk = 4096; }},
      {"tiled grid > 2^31 dtype=0", VMC_E_DTYPE, [](AttnFwdProblem& p) { p.B = 1 << 20; p.H = 64; p.Tq = p.Tk = 4096; p.dtype16 = 0; }},
      {"q=0 B=0", VMC_E_ARG, [](AttnFwdProblem& p) { p.q = nullptr; p.B = 0; }},
      {"B=0 dh=60", VMC_E_ARG, [](AttnFwdProblem& p) { p.B = 0; p.dh = 60; }},
      {"dh=60 ldq=1540", VMC_E_SHAPE, [](AttnFwdProblem& p) { p.dh = 60; p.ldq = 1540; }},
      {"ldq=1540 q+8", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.ldq = 1540; p.q = cp(0x100008); }},
      {"q+8 dtype=0", VMC_E_ALIGN, [](AttnFwdProblem& p) { p.q = cp(0x100008); p.dtype16 = 0; }},
      {"(valid)", 0, [](AttnFwdProblem& p) { (void)p; }},
  };
  for (const FwdErr& c : kFwdErr) {
    AttnFwdProblem p = fwd(8, 8, 64, 64, 64);
    c.bad(p);
    const int rc = attn_fwd_route(p).rc;
    CHECK(rc == c.want, "fwd %s: %d, want %d", c.what, rc, c.want);
    ++cases;
  }

  struct BwdErr { const char* what; int want; void (*bad)(AttnBwdProblem&); };
  static const BwdErr kBwdErr[] = {      // on B = H = 8, T = 64, dh 64 (attn_bwd_mfma_kernel)
      {"q=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.q = nullptr; }},
      {"k=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.k = nullptr; }},
      {"v=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.v = nullptr; }},
      {"out=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.out = nullptr; }},
      {"dout=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.dout = nullptr; }},
      {"lse=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.lse = nullptr; }},
      {"dq=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.dq = nullptr; }},
      {"dk=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.dk = nullptr; }},
      {"dv=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.dv = nullptr; }},
      {"workspace=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.workspace = nullptr; }},
      {"B=0", VMC_E_ARG, [](AttnBwdProblem& p) { p.B = 0; }},
      {"Tk=-1", VMC_E_ARG, [](AttnBwdProblem& p) { p.Tk = -1; }},
      {"dh=60", VMC_E_SHAPE, [](AttnBwdProblem& p) { p.dh = 60; }},
      {"dh=136", VMC_E_SHAPE, [](AttnBwdProblem& p) { p.dh = 136; }},
      {"ldk=1028", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.ldk = 1028; }},
      {"ldo=516", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.ldo = 516; }},
      {"workspace short", VMC_E_ARG, [](AttnBwdProblem& p) { p.workspace_bytes -= 1; }},
      {"q+8", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.q = cp(0x100008); }},
      {"k+8", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.k = cp(0x200008); }},
      {"v+8", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.v = cp(0x300008); }},
      {"dout+8", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.dout = cp(0x500008); }},
      {"dtype=0 (in LDS)", VMC_E_DTYPE, [](AttnBwdProblem& p) { p.dtype16 = 0; }},
      {"dtype=3 T=289 (tiled)", VMC_E_DTYPE, [](AttnBwdProblem& p) { p.dtype16 = 3; p.Tq = p.Tk = 289; p.workspace_bytes = (size_t)-1; }},
      {"dtype=0 dh=32 (scalar)", VMC_E_DTYPE, [](AttnBwdProblem& p) { p.dtype16 = 0; p.dh = 32; }},
      {"dtype=0 dh=32 Tk=2049", VMC_E_SHAPE, [](AttnBwdProblem& p) { p.dtype16 = 0; p.dh = 32; p.Tk = 2049; }},
      {"tiled grid > 2^31", VMC_E_SHAPE, [](AttnBwdProblem& p) { p.B = 1 << 20; p.H = 64; p.Tq = p.Tk = 4096; p.workspace_bytes = (size_t)-1; }},
      {"tiled grid > 2^31 dtype=0", VMC_E_DTYPE,
       [](AttnBwdProblem& p) { p.B = 1 << 20; p.H = 64; p.Tq = p.Tk = 4096; p.workspace_bytes = (size_t)-1; p.dtype16 = 0; }},
      {"workspace short dh=60", VMC_E_SHAPE, [](AttnBwdProblem& p) { p.workspace_bytes -= 1; p.dh = 60; }},
      {"workspace short q+8", VMC_E_ARG, [](AttnBwdProblem& p) { p.workspace_bytes -= 1; p.q = cp(0x100008); }},
      {"dout+8 dtype=0", VMC_E_ALIGN, [](AttnBwdProblem& p) { p.dout = cp(0x500008); p.dtype16 = 0; }},
      {"(valid)", 0, [](AttnBwdProblem& p) { (void)p; }},
  };
  for (const BwdErr& c : kBwdErr) {
    AttnBwdProblem p = bwd(8, 8, 64, 64, 64);
    c.bad(p);
    const int rc = attn_bwd_route(p).rc;
    CHECK(rc == c.want, "bwd %s: %d, want %d", c.what, rc, c.want);
    ++cases;
  }

  // every instantiation is reached by some case (none is kept without a route to it)
  for (int i = 0; i < kAttnVitInstCount; ++i) CHECK(vit_seen[i], "kAttnVitInsts[%d] is never routed", i);
  for (int i = 0; i < kAttnInstCount; ++i) CHECK(inst_seen[i], "kAttnInsts[%d] is never routed", i);

  // the switch keeps its name and default
  unsetenv("VMC_ATTN_VARIANT");
  CHECK(attn_overrides_from_env().variant == 1, "VMC_ATTN_VARIANT default");
  setenv("VMC_ATTN_VARIANT", "21", 1);
  CHECK(attn_overrides_from_env().variant == 21, "VMC_ATTN_VARIANT=21");

  if (fails) {
    printf("%d FAILED\n", fails);
    return 1;
  }
  printf("OK: %d routing cases\n", cases);
  return 0;
}
