// Host test of the GEMM dispatch (vimo_clip_amd/csrc/gemm_route.h): the plans for the shapes the models issue, every
// vmc_linear_variant value and every builder switch, the argument checks, the weight-gradient and split-K routes and the
// workspace sizes.  The expected plans were recorded from the dispatch as it stood before it moved into gemm_route.h, so a
// change of routing shows up here instead of only as a different time on the GPU.  Built with g++ by tests/test_host_gemm_route.py.
//
// A plan reads "kernel[row0+rows] ...": tile<MT,WM,WN,NS,KS,U> = gemm_kernel, g8 = gemm8_kernel (one tile per workgroup),
// g8p<act,bias,zout> / g8p32<...> = the persistent walks.  Problem flags: b bias, z pre-activation side output, r16 / r32
// residual, o32 f32 output, q / g / r QuickGELU / erf-GELU / ReLU, lda= ldw= org= (out_row_group) rrm= (res_row_mod).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../vimo_clip_amd/csrc/gemm_route.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 30) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static const void* ptr(uintptr_t a) { return (const void*)a; }

static GemmProblem prob(int M, int N, int K, const char* flags) {
  GemmProblem p = {ptr(0x10000), ptr(0x20000), nullptr, nullptr, ptr(0x30000), nullptr, M, N, K, K, K, N, 0, 0, VMC_ACT_NONE, 1.0f,
                   VMC_BF16, 0, 0, 0, VMC_BF16};
  char buf[128];
  snprintf(buf, sizeof buf, "%s", flags);
  for (char* t = strtok(buf, " "); t; t = strtok(nullptr, " ")) {
    const char* eq = strchr(t, '=');
    const int v = eq ? atoi(eq + 1) : 0;
    if (!strcmp(t, "b")) p.bias = ptr(0x50000);
    else if (!strcmp(t, "z")) { p.Z = ptr(0x60000); p.ldz = N; }
    else if (!strcmp(t, "r16") || !strcmp(t, "r32")) { p.res = ptr(0x40000); p.ldres = N; p.res_dtype = t[1] == '3' ? VMC_F32 : VMC_BF16; }
    else if (!strcmp(t, "o32")) p.out_dtype = VMC_F32;
    else if (!strcmp(t, "q")) p.act = VMC_ACT_QUICKGELU;
    else if (!strcmp(t, "g")) p.act = VMC_ACT_GELU_ERF;
    else if (!strcmp(t, "r")) p.act = VMC_ACT_RELU;
    else if (!strncmp(t, "lda=", 4)) p.lda = v;
    else if (!strncmp(t, "ldw=", 4)) p.ldw = v;
    else if (!strncmp(t, "org=", 4)) p.out_row_group = v;
    else if (!strncmp(t, "rrm=", 4)) p.res_row_mod = v;
    else { printf("bad flag %s\n", t); exit(2); }
  }
  return p;
}

static GemmOverrides overrides(const char* spec) {
  GemmOverrides o;
  char buf[128];
  snprintf(buf, sizeof buf, "%s", spec);
  for (char* t = strtok(buf, " "); t; t = strtok(nullptr, " ")) {
    const int v = atoi(strchr(t, '=') + 1);
    if (!strncmp(t, "cfg=", 4)) o.cfg = v;
    else if (!strncmp(t, "ks=", 3)) o.ks = v != 0;
    else if (!strncmp(t, "u=", 2)) o.u = v;
    else if (!strncmp(t, "mfma32=", 7)) o.mfma32 = v != 0;
    else if (!strncmp(t, "gc=", 3)) o.gc = v;
    else if (!strncmp(t, "tn256=", 6)) o.tn256 = v != 0;
    else if (!strncmp(t, "tn256_min_pairs=", 16)) o.tn256_min_pairs = v;
    else { printf("bad override %s\n", t); exit(2); }
  }
  return o;
}

static std::string plan_str(const GemmPlan& pl) {
  std::string s;
  char b[96];
  for (int i = 0; i < pl.n; ++i) {
    const GemmLaunch& l = pl.launch[i];
    if (l.family == GEMM_TILE) {
      const GemmTileCfg& c = kGemmTileCfgs[l.cfg];
      snprintf(b, sizeof b, "tile<%d,%d,%d,%d,%d,%d>", c.mt, c.wm, c.wn, c.ns, c.ks, c.u);
    } else if (l.family == GEMM_8P) {
      const Gemm8pInst& k = kGemm8pInsts[l.cfg];
      snprintf(b, sizeof b, "%s<%d,%d,%d>", k.mfma32 ? "g8p32" : "g8p", k.act, (int)k.bias, (int)k.zout);
    } else {
      snprintf(b, sizeof b, "g8");
    }
    s += (i ? " " : "") + std::string(b);
    snprintf(b, sizeof b, "[%d+%d]", l.row0, l.rows);
    s += b;
  }
  return s;
}

// every launch names an instantiated kernel and meets what its launcher checks at run time
static void check_plan(const char* name, const GemmProblem& p, const GemmPlan& pl) {
  CHECK(pl.n == 1 || pl.n == 2, "%s: %d launches", name, pl.n);
  int next = 0;
  for (int i = 0; i < pl.n; ++i) {
    const GemmLaunch& l = pl.launch[i];
    CHECK(l.row0 == next && l.rows > 0, "%s: launch %d covers [%d, +%d)", name, i, l.row0, l.rows);
    next = l.row0 + l.rows;
    if (l.family == GEMM_TILE) {
      CHECK(l.cfg >= 0 && l.cfg < kGemmTileCfgCount, "%s: tile config %d", name, l.cfg);
      const GemmTileCfg& c = kGemmTileCfgs[l.cfg];
      CHECK(!c.none_only || p.act == VMC_ACT_NONE, "%s: sweep tile for act %d is not instantiated", name, p.act);
      CHECK((p.K / 64) % c.u == 0, "%s: (K/64) %% U != 0", name);
      CHECK(c.ks == 1 || c.ns > 2, "%s: K-slice groups without a ring", name);
    } else if (l.family == GEMM_8P) {
      CHECK(l.cfg >= 0 && l.cfg < kGemm8pInstCount, "%s: persistent instance %d", name, l.cfg);
      const Gemm8pInst& k = kGemm8pInsts[l.cfg];
      CHECK(k.act == p.act && k.bias == (p.bias != nullptr) && k.zout == (p.Z != nullptr), "%s: epilogue mismatch", name);
      CHECK(l.rows % 256 == 0 && p.N % 256 == 0 && p.K % 128 == 0, "%s: persistent walk on partial tiles", name);
    } else {
      CHECK(l.family == GEMM_8 && l.cfg == 0 && p.K % 128 == 0, "%s: 8-phase launch", name);
    }
  }
  CHECK(next == p.M, "%s: launches cover %d of %d rows", name, next, p.M);
}

struct GemmCase {
  const char* name;
  int M, N, K;
  const char* flags;
  int variant;
  const char* ov;
  const char* want;
};
static const GemmCase kGemmCases[] = {
    {"vitl qkv", 65792, 3072, 1024, "b", 1, "", "g8p<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl kv", 65792, 2048, 1024, "b", 1, "", "g8p<0,1,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl out_proj", 65792, 1024, 1024, "b", 1, "", "g8p<0,1,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl out_proj +res f32", 65792, 1024, 1024, "b r32 o32", 1, "", "g8[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu", 65792, 4096, 1024, "b q", 1, "", "g8p<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu preact", 65792, 4096, 1024, "b q z", 1, "", "g8p<1,1,1>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_proj", 65792, 1024, 4096, "b", 1, "", "g8p<0,1,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl c_proj +res f32", 65792, 1024, 4096, "b r32 o32", 1, "", "g8[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl cls q", 256, 1024, 1024, "b lda=263168", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl cls out_proj +res", 256, 1024, 1024, "b r32 o32", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl cls c_fc", 256, 4096, 1024, "b q", 1, "", "tile<2,2,1,8,1,4>[0+256]"},
    {"vitl cls c_proj +res", 256, 1024, 4096, "b r32 o32", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl cls out_proj", 256, 1024, 1024, "b", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl cls c_proj", 256, 1024, 4096, "b", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl proj f32", 256, 768, 1024, "o32", 1, "", "tile<1,2,1,8,1,4>[0+256]"},
    {"vitl patch remap", 65536, 1024, 640, "b r32 o32 org=256 rrm=256", 1, "", "g8[0+65536]"},
    {"vitb student patch remap", 25088, 768, 3072, "b r32 o32 org=49 rrm=49", 1, "", "g8[0+25088]"},
    {"student qkv", 25600, 2304, 768, "b", 1, "", "g8p<0,1,0>[0+25600]"},
    {"student out_proj +res", 25600, 768, 768, "b r32 o32", 1, "", "g8[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"student c_fc", 25600, 3072, 768, "b q", 1, "", "g8p<1,1,0>[0+25600]"},
    {"student c_fc preact", 25600, 3072, 768, "b q z", 1, "", "g8p<1,1,1>[0+25600]"},
    {"student c_proj +res", 25600, 768, 3072, "b r32 o32", 1, "", "g8[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"student c_proj", 25600, 768, 3072, "b", 1, "", "g8p<0,1,0>[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"student dgrad qkv", 25600, 768, 2304, "", 1, "", "g8p<0,0,0>[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"student dgrad c_fc", 25600, 768, 3072, "", 1, "", "g8p<0,0,0>[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"student dgrad c_proj", 25600, 3072, 768, "", 1, "", "g8p<0,0,0>[0+25600]"},
    {"student dgrad out_proj", 25600, 768, 768, "", 1, "", "g8p<0,0,0>[0+21760] tile<4,2,2,2,1,1>[21760+3840]"},
    {"vitl dgrad c_proj", 65792, 4096, 1024, "", 1, "", "g8p<0,0,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad c_fc", 65792, 1024, 4096, "", 1, "", "g8p<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad qkv", 65792, 1024, 3072, "", 1, "", "g8p<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"dgrad K-padded ldw", 25600, 768, 832, "ldw=896", 1, "", "tile<8,2,4,2,1,1>[0+25600]"},
    {"dgrad padded K=640", 8192, 512, 640, "", 1, "", "tile<4,2,2,2,1,1>[0+8192]"},
    {"tfam B=8 D=512 qkv", 128, 1536, 512, "b", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=512 out", 128, 512, 512, "b r16", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=512 ff1 relu", 128, 2048, 512, "b r", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=512 ff2", 128, 512, 2048, "b r16", 1, "", "tile<1,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=512 cls hidden", 8, 256, 512, "b r", 1, "", "tile<2,2,1,8,1,4>[0+8]"},
    {"tfam B=8 D=512 cls out", 8, 140, 256, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+8]"},
    {"tfam B=8 D=512 ff1 train preact relu", 128, 2048, 512, "b r z", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=768 qkv", 128, 2304, 768, "b", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=768 out", 128, 768, 768, "b r16", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=768 ff1 relu", 128, 2048, 768, "b r", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=768 ff2", 128, 768, 2048, "b r16", 1, "", "tile<1,2,1,8,1,4>[0+128]"},
    {"tfam B=8 D=768 cls hidden", 8, 384, 768, "b r", 1, "", "tile<2,2,1,8,1,4>[0+8]"},
    {"tfam B=8 D=768 cls out", 8, 140, 384, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+8]"},
    {"tfam B=8 D=768 ff1 train preact relu", 128, 2048, 768, "b r z", 1, "", "tile<2,2,1,8,1,4>[0+128]"},
    {"tfam B=64 D=512 qkv", 1024, 1536, 512, "b", 1, "", "tile<2,2,1,4,1,1>[0+1024]"},
    {"tfam B=64 D=512 out", 1024, 512, 512, "b r16", 1, "", "tile<2,2,1,8,1,4>[0+1024]"},
    {"tfam B=64 D=512 ff1 relu", 1024, 2048, 512, "b r", 1, "", "tile<4,2,2,2,1,1>[0+1024]"},
    {"tfam B=64 D=512 ff2", 1024, 512, 2048, "b r16", 1, "", "tile<1,2,1,8,1,4>[0+1024]"},
    {"tfam B=64 D=512 cls hidden", 64, 256, 512, "b r", 1, "", "tile<2,2,1,8,1,4>[0+64]"},
    {"tfam B=64 D=512 cls out", 64, 140, 256, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+64]"},
    {"tfam B=64 D=512 ff1 train preact relu", 1024, 2048, 512, "b r z", 1, "", "tile<4,2,2,2,1,1>[0+1024]"},
    {"tfam B=64 D=768 qkv", 1024, 2304, 768, "b", 1, "", "tile<4,2,2,2,1,1>[0+1024]"},
    {"tfam B=64 D=768 out", 1024, 768, 768, "b r16", 1, "", "tile<2,2,1,8,1,4>[0+1024]"},
    {"tfam B=64 D=768 ff1 relu", 1024, 2048, 768, "b r", 1, "", "tile<4,2,2,2,1,1>[0+1024]"},
    {"tfam B=64 D=768 ff2", 1024, 768, 2048, "b r16", 1, "", "tile<2,2,1,8,1,4>[0+1024]"},
    {"tfam B=64 D=768 cls hidden", 64, 384, 768, "b r", 1, "", "tile<2,2,1,8,1,4>[0+64]"},
    {"tfam B=64 D=768 cls out", 64, 140, 384, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+64]"},
    {"tfam B=64 D=768 ff1 train preact relu", 1024, 2048, 768, "b r z", 1, "", "tile<4,2,2,2,1,1>[0+1024]"},
    {"tfam B=512 D=512 qkv", 8192, 1536, 512, "b", 1, "", "g8p<0,1,0>[0+8192]"},
    {"tfam B=512 D=512 out", 8192, 512, 512, "b r16", 1, "", "tile<4,2,2,2,1,1>[0+8192]"},
    {"tfam B=512 D=512 ff1 relu", 8192, 2048, 512, "b r", 1, "", "g8p<3,1,0>[0+8192]"},
    {"tfam B=512 D=512 ff2", 8192, 512, 2048, "b r16", 1, "", "tile<4,2,2,2,1,1>[0+8192]"},
    {"tfam B=512 D=512 cls hidden", 512, 256, 512, "b r", 1, "", "tile<2,2,1,8,1,4>[0+512]"},
    {"tfam B=512 D=512 cls out", 512, 140, 256, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+512]"},
    {"tfam B=512 D=512 ff1 train preact relu", 8192, 2048, 512, "b r z", 1, "", "g8[0+8192]"},
    {"tfam B=512 D=768 qkv", 8192, 2304, 768, "b", 1, "", "g8p<0,1,0>[0+7168] tile<4,2,2,2,1,1>[7168+1024]"},
    {"tfam B=512 D=768 out", 8192, 768, 768, "b r16", 1, "", "tile<4,2,2,2,1,1>[0+8192]"},
    {"tfam B=512 D=768 ff1 relu", 8192, 2048, 768, "b r", 1, "", "g8p<3,1,0>[0+8192]"},
    {"tfam B=512 D=768 ff2", 8192, 768, 2048, "b r16", 1, "", "tile<4,2,2,2,1,1>[0+8192]"},
    {"tfam B=512 D=768 cls hidden", 512, 384, 768, "b r", 1, "", "tile<2,2,1,8,1,4>[0+512]"},
    {"tfam B=512 D=768 cls out", 512, 140, 384, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+512]"},
    {"tfam B=512 D=768 ff1 train preact relu", 8192, 2048, 768, "b r z", 1, "", "g8[0+8192]"},
    {"tfam B=4096 D=512 qkv", 65536, 1536, 512, "b", 1, "", "g8p<0,1,0>[0+65536]"},
    {"tfam B=4096 D=512 out", 65536, 512, 512, "b r16", 1, "", "g8[0+65536]"},
    {"tfam B=4096 D=512 ff1 relu", 65536, 2048, 512, "b r", 1, "", "g8p<3,1,0>[0+65536]"},
    {"tfam B=4096 D=512 ff2", 65536, 512, 2048, "b r16", 1, "", "g8[0+65536]"},
    {"tfam B=4096 D=512 cls hidden", 4096, 256, 512, "b r", 1, "", "tile<2,2,1,8,1,4>[0+4096]"},
    {"tfam B=4096 D=512 cls out", 4096, 140, 256, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+4096]"},
    {"tfam B=4096 D=512 ff1 train preact relu", 65536, 2048, 512, "b r z", 1, "", "g8[0+65536]"},
    {"tfam B=4096 D=768 qkv", 65536, 2304, 768, "b", 1, "", "g8p<0,1,0>[0+65536]"},
    {"tfam B=4096 D=768 out", 65536, 768, 768, "b r16", 1, "", "g8[0+65536]"},
    {"tfam B=4096 D=768 ff1 relu", 65536, 2048, 768, "b r", 1, "", "g8p<3,1,0>[0+65536]"},
    {"tfam B=4096 D=768 ff2", 65536, 768, 2048, "b r16", 1, "", "g8[0+65536]"},
    {"tfam B=4096 D=768 cls hidden", 4096, 384, 768, "b r", 1, "", "tile<2,2,1,4,1,1>[0+4096]"},
    {"tfam B=4096 D=768 cls out", 4096, 140, 384, "b o32", 1, "", "tile<2,2,1,4,1,1>[0+4096]"},
    {"tfam B=4096 D=768 ff1 train preact relu", 65536, 2048, 768, "b r z", 1, "", "g8[0+65536]"},
    {"qkv 4096x2304x768 (129-191 tiles)", 4096, 2304, 768, "b", 1, "", "g8[0+4096]"},
    {"4096x2048x768 (128 tiles)", 4096, 2048, 768, "b", 1, "", "tile<4,2,2,2,1,1>[0+4096]"},
    {"4096x2304x768 gelu", 4096, 2304, 768, "b g", 1, "", "g8[0+4096]"},
    {"vitl qkv variant 0", 65792, 3072, 1024, "b", 0, "", "tile<8,2,4,2,1,1>[0+65792]"},
    {"vitl c_fc quickgelu variant 0", 65792, 4096, 1024, "b q", 0, "", "tile<8,2,4,2,1,1>[0+65792]"},
    {"student qkv variant 0", 25600, 2304, 768, "b", 0, "", "tile<8,2,4,2,1,1>[0+25600]"},
    {"4096x2304x768 variant 0", 4096, 2304, 768, "b", 0, "", "tile<4,2,2,2,1,1>[0+4096]"},
    {"vitl c_fc relu variant 0", 65792, 4096, 1024, "b r", 0, "", "tile<8,2,4,2,1,1>[0+65792]"},
    {"vitl dgrad variant 0", 65792, 1024, 3072, "", 0, "", "tile<8,2,4,2,1,1>[0+65792]"},
    {"vitl qkv variant 1", 65792, 3072, 1024, "b", 1, "", "g8p<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu variant 1", 65792, 4096, 1024, "b q", 1, "", "g8p<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"student qkv variant 1", 25600, 2304, 768, "b", 1, "", "g8p<0,1,0>[0+25600]"},
    {"4096x2304x768 variant 1", 4096, 2304, 768, "b", 1, "", "g8[0+4096]"},
    {"vitl c_fc relu variant 1", 65792, 4096, 1024, "b r", 1, "", "g8p<3,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad variant 1", 65792, 1024, 3072, "", 1, "", "g8p<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl qkv variant 2", 65792, 3072, 1024, "b", 2, "", "g8p<0,1,0>[0+65792]"},
    {"vitl c_fc quickgelu variant 2", 65792, 4096, 1024, "b q", 2, "", "g8p<1,1,0>[0+65792]"},
    {"student qkv variant 2", 25600, 2304, 768, "b", 2, "", "g8p<0,1,0>[0+25600]"},
    {"4096x2304x768 variant 2", 4096, 2304, 768, "b", 2, "", "g8[0+4096]"},
    {"vitl c_fc relu variant 2", 65792, 4096, 1024, "b r", 2, "", "g8p<3,1,0>[0+65792]"},
    {"vitl dgrad variant 2", 65792, 1024, 3072, "", 2, "", "g8p<0,0,0>[0+65792]"},
    {"vitl qkv variant 3", 65792, 3072, 1024, "b", 3, "", "g8p<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu variant 3", 65792, 4096, 1024, "b q", 3, "", "g8p<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"student qkv variant 3", 25600, 2304, 768, "b", 3, "", "g8p<0,1,0>[0+25600]"},
    {"4096x2304x768 variant 3", 4096, 2304, 768, "b", 3, "", "g8[0+4096]"},
    {"vitl c_fc relu variant 3", 65792, 4096, 1024, "b r", 3, "", "g8p<3,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad variant 3", 65792, 1024, 3072, "", 3, "", "g8p<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl qkv variant 4", 65792, 3072, 1024, "b", 4, "", "g8[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu variant 4", 65792, 4096, 1024, "b q", 4, "", "g8[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"student qkv variant 4", 25600, 2304, 768, "b", 4, "", "g8[0+25600]"},
    {"4096x2304x768 variant 4", 4096, 2304, 768, "b", 4, "", "g8[0+4096]"},
    {"vitl c_fc relu variant 4", 65792, 4096, 1024, "b r", 4, "", "g8[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad variant 4", 65792, 1024, 3072, "", 4, "", "g8[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"vitl qkv variant 5", 65792, 3072, 1024, "b", 5, "", "g8p32<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl c_fc quickgelu variant 5", 65792, 4096, 1024, "b q", 5, "", "g8p32<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"student qkv variant 5", 25600, 2304, 768, "b", 5, "", "g8p32<0,1,0>[0+25600]"},
    {"4096x2304x768 variant 5", 4096, 2304, 768, "b", 5, "", "g8[0+4096]"},
    {"vitl c_fc relu variant 5", 65792, 4096, 1024, "b r", 5, "", "g8p<3,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"vitl dgrad variant 5", 65792, 1024, 3072, "", 5, "", "g8p32<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"cfg=1 none", 1024, 512, 2048, "b r16", 1, "cfg=1", "tile<4,2,2,3,1,1>[0+1024]"},
    {"cfg=1 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=1", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=1 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=1", "g8p<0,1,0>[0+65536] tile<4,2,2,3,1,1>[65536+256]"},
    {"cfg=2 none", 1024, 512, 2048, "b r16", 1, "cfg=2", "tile<4,2,2,4,1,1>[0+1024]"},
    {"cfg=2 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=2", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=2 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=2", "g8p<0,1,0>[0+65536] tile<4,2,2,4,1,1>[65536+256]"},
    {"cfg=3 none", 1024, 512, 2048, "b r16", 1, "cfg=3", "tile<4,2,1,4,1,1>[0+1024]"},
    {"cfg=3 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=3", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=3 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=3", "g8p<0,1,0>[0+65536] tile<4,2,1,4,1,1>[65536+256]"},
    {"cfg=4 none", 1024, 512, 2048, "b r16", 1, "cfg=4", "tile<2,2,2,4,1,1>[0+1024]"},
    {"cfg=4 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=4", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=4 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=4", "g8p<0,1,0>[0+65536] tile<2,2,2,4,1,1>[65536+256]"},
    {"cfg=5 none", 1024, 512, 2048, "b r16", 1, "cfg=5", "tile<2,2,1,4,1,1>[0+1024]"},
    {"cfg=5 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=5", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=5 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=5", "g8p<0,1,0>[0+65536] tile<2,2,1,4,1,1>[65536+256]"},
    {"cfg=6 none", 1024, 512, 2048, "b r16", 1, "cfg=6", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=6 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=6", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=6 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=6", "g8p<0,1,0>[0+65536] tile<4,2,2,2,1,1>[65536+256]"},
    {"cfg=7 none", 1024, 512, 2048, "b r16", 1, "cfg=7", "tile<4,2,1,6,1,1>[0+1024]"},
    {"cfg=7 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=7", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=7 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=7", "g8p<0,1,0>[0+65536] tile<4,2,1,6,1,1>[65536+256]"},
    {"cfg=8 none", 1024, 512, 2048, "b r16", 1, "cfg=8", "tile<2,2,2,6,1,1>[0+1024]"},
    {"cfg=8 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=8", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=8 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=8", "g8p<0,1,0>[0+65536] tile<2,2,2,6,1,1>[65536+256]"},
    {"cfg=9 none", 1024, 512, 2048, "b r16", 1, "cfg=9", "tile<8,2,2,2,1,1>[0+1024]"},
    {"cfg=9 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=9", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=9 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=9", "g8p<0,1,0>[0+65536] tile<8,2,2,2,1,1>[65536+256]"},
    {"cfg=10 none", 1024, 512, 2048, "b r16", 1, "cfg=10", "tile<8,2,2,3,1,1>[0+1024]"},
    {"cfg=10 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=10", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=10 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=10", "g8p<0,1,0>[0+65536] tile<8,2,2,3,1,1>[65536+256]"},
    {"cfg=11 none", 1024, 512, 2048, "b r16", 1, "cfg=11", "tile<4,2,4,2,1,1>[0+1024]"},
    {"cfg=11 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=11", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=11 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=11", "g8p<0,1,0>[0+65536] tile<4,2,4,2,1,1>[65536+256]"},
    {"cfg=12 none", 1024, 512, 2048, "b r16", 1, "cfg=12", "tile<1,2,1,8,1,4>[0+1024]"},
    {"cfg=12 relu (no sweep)", 1024, 2048, 512, "b r", 1, "cfg=12", "tile<4,2,2,2,1,1>[0+1024]"},
    {"cfg=12 tail of vitl c_proj", 65792, 1024, 4096, "b", 1, "cfg=12", "g8p<0,1,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"ks=1 cls c_proj", 256, 1024, 4096, "b", 1, "ks=1", "tile<1,2,1,3,4,1>[0+256]"},
    {"ks=1 cls qkv", 256, 3072, 1024, "b", 1, "ks=1", "tile<2,2,1,4,2,1>[0+256]"},
    {"ks=1 tfam B=8 ff2", 128, 768, 2048, "b", 1, "ks=1", "tile<1,2,1,3,4,1>[0+128]"},
    {"ks=1 vitl qkv", 65792, 3072, 1024, "b", 1, "ks=1", "g8p<0,1,0>[0+65536] tile<2,2,1,4,2,1>[65536+256]"},
    {"ks=1 512x512x448", 512, 512, 448, "b", 1, "ks=1", "tile<2,2,1,4,1,1>[0+512]"},
    {"u=1 cls c_proj", 256, 1024, 4096, "b", 1, "u=1", "tile<1,2,1,4,1,1>[0+256]"},
    {"u=1 cls qkv", 256, 3072, 1024, "b", 1, "u=1", "tile<2,2,1,4,1,1>[0+256]"},
    {"u=1 tfam B=8 ff2", 128, 768, 2048, "b", 1, "u=1", "tile<1,2,1,4,1,1>[0+128]"},
    {"u=1 vitl qkv", 65792, 3072, 1024, "b", 1, "u=1", "g8p<0,1,0>[0+65536] tile<2,2,1,4,1,1>[65536+256]"},
    {"u=1 512x512x448", 512, 512, 448, "b", 1, "u=1", "tile<2,2,1,4,1,1>[0+512]"},
    {"u=2 cls c_proj", 256, 1024, 4096, "b", 1, "u=2", "tile<1,2,1,6,1,2>[0+256]"},
    {"u=2 cls qkv", 256, 3072, 1024, "b", 1, "u=2", "tile<2,2,1,6,1,2>[0+256]"},
    {"u=2 tfam B=8 ff2", 128, 768, 2048, "b", 1, "u=2", "tile<1,2,1,6,1,2>[0+128]"},
    {"u=2 vitl qkv", 65792, 3072, 1024, "b", 1, "u=2", "g8p<0,1,0>[0+65536] tile<2,2,1,6,1,2>[65536+256]"},
    {"u=2 512x512x448", 512, 512, 448, "b", 1, "u=2", "tile<2,2,1,4,1,1>[0+512]"},
    {"u=3 cls c_proj", 256, 1024, 4096, "b", 1, "u=3", "tile<1,2,1,4,1,1>[0+256]"},
    {"u=3 cls qkv", 256, 3072, 1024, "b", 1, "u=3", "tile<2,2,1,4,1,1>[0+256]"},
    {"u=3 tfam B=8 ff2", 128, 768, 2048, "b", 1, "u=3", "tile<1,2,1,4,1,1>[0+128]"},
    {"u=3 vitl qkv", 65792, 3072, 1024, "b", 1, "u=3", "g8p<0,1,0>[0+65536] tile<2,2,1,4,1,1>[65536+256]"},
    {"u=3 512x512x448", 512, 512, 448, "b", 1, "u=3", "tile<2,2,1,4,1,1>[0+512]"},
    {"ks=1 u=2 cls c_proj", 256, 1024, 4096, "b", 1, "ks=1 u=2", "tile<1,2,1,3,4,1>[0+256]"},
    {"ks=1 u=2 cls qkv", 256, 3072, 1024, "b", 1, "ks=1 u=2", "tile<2,2,1,4,2,1>[0+256]"},
    {"ks=1 u=2 tfam B=8 ff2", 128, 768, 2048, "b", 1, "ks=1 u=2", "tile<1,2,1,3,4,1>[0+128]"},
    {"ks=1 u=2 vitl qkv", 65792, 3072, 1024, "b", 1, "ks=1 u=2", "g8p<0,1,0>[0+65536] tile<2,2,1,4,2,1>[65536+256]"},
    {"ks=1 u=2 512x512x448", 512, 512, 448, "b", 1, "ks=1 u=2", "tile<2,2,1,4,1,1>[0+512]"},
    {"mfma32=1 vitl qkv", 65792, 3072, 1024, "b", 1, "mfma32=1", "g8p32<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"mfma32=1 vitl c_fc", 65792, 4096, 1024, "b q", 1, "mfma32=1", "g8p32<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"mfma32=1 vitl c_fc preact", 65792, 4096, 1024, "b q z", 1, "mfma32=1", "g8p<1,1,1>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"mfma32=1 vitl dgrad", 65792, 1024, 3072, "", 1, "mfma32=1", "g8p32<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"mfma32=1 vitl c_fc relu", 65792, 4096, 1024, "b r", 1, "mfma32=1", "g8p<3,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"gc=2 vitl qkv", 65792, 3072, 1024, "b", 1, "gc=2", "g8p<0,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"gc=2 vitl c_fc", 65792, 4096, 1024, "b q", 1, "gc=2", "g8p<1,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"gc=2 vitl c_fc preact", 65792, 4096, 1024, "b q z", 1, "gc=2", "g8p<1,1,1>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
    {"gc=2 vitl dgrad", 65792, 1024, 3072, "", 1, "gc=2", "g8p<0,0,0>[0+65536] tile<1,2,1,8,1,4>[65536+256]"},
    {"gc=2 vitl c_fc relu", 65792, 4096, 1024, "b r", 1, "gc=2", "g8p<3,1,0>[0+65536] tile<2,2,1,8,1,4>[65536+256]"},
};

struct ErrCase {
  const char* what;
  int want;
  void (*bad)(GemmProblem&, int&);
};
static const ErrCase kErrCases[] = {      // one bad argument each on 1024 x 512 x 1024 with a bias, in the order they are checked
    {"variant=-1", VMC_E_ARG, [](GemmProblem& p, int& v) { v = -1; (void)p; (void)v; }},
    {"variant=6", VMC_E_ARG, [](GemmProblem& p, int& v) { v = 6; (void)p; (void)v; }},
    {"A=0", VMC_E_ARG, [](GemmProblem& p, int& v) { p.A = nullptr; (void)p; (void)v; }},
    {"W=0", VMC_E_ARG, [](GemmProblem& p, int& v) { p.W = nullptr; (void)p; (void)v; }},
    {"C=0", VMC_E_ARG, [](GemmProblem& p, int& v) { p.C = nullptr; (void)p; (void)v; }},
    {"M=0", VMC_E_ARG, [](GemmProblem& p, int& v) { p.M = 0; (void)p; (void)v; }},
    {"N=-4", VMC_E_ARG, [](GemmProblem& p, int& v) { p.N = -4; (void)p; (void)v; }},
    {"K=0", VMC_E_ARG, [](GemmProblem& p, int& v) { p.K = 0; (void)p; (void)v; }},
    {"z ldz=508", VMC_E_ARG, [](GemmProblem& p, int& v) { p.Z = ptr(0x60000); p.ldz = 512; p.ldz = 508; (void)p; (void)v; }},
    {"z ldz=514", VMC_E_ARG, [](GemmProblem& p, int& v) { p.Z = ptr(0x60000); p.ldz = 512; p.ldz = 514; (void)p; (void)v; }},
    {"z Zoff=8", VMC_E_ARG, [](GemmProblem& p, int& v) { p.Z = ptr(0x60000); p.ldz = 512; p.Z = ptr(0x60000 + 8); (void)p; (void)v; }},
    {"z org=4", VMC_E_ARG, [](GemmProblem& p, int& v) { p.Z = ptr(0x60000); p.ldz = 512; p.out_row_group = 4; (void)p; (void)v; }},
    {"dt=0", VMC_E_DTYPE, [](GemmProblem& p, int& v) { p.dtype16 = 0; (void)p; (void)v; }},
    {"dt=3", VMC_E_DTYPE, [](GemmProblem& p, int& v) { p.dtype16 = 3; (void)p; (void)v; }},
    {"K=96", VMC_E_SHAPE, [](GemmProblem& p, int& v) { p.K = 96; (void)p; (void)v; }},
    {"N=6", VMC_E_SHAPE, [](GemmProblem& p, int& v) { p.N = 6; (void)p; (void)v; }},
    {"lda=1028", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.lda = 1028; (void)p; (void)v; }},
    {"ldw=1030", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.ldw = 1030; (void)p; (void)v; }},
    {"ldc=514", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.ldc = 514; (void)p; (void)v; }},
    {"r16 ldres=510", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.res = ptr(0x40000); p.ldres = 512; p.res_dtype = VMC_BF16; p.ldres = 510; (void)p; (void)v; }},
    {"Aoff=8", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.A = ptr(0x10000 + 8); (void)p; (void)v; }},
    {"Woff=4", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.W = ptr(0x20000 + 4); (void)p; (void)v; }},
    {"Coff=2", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.C = ptr(0x30000 + 2); (void)p; (void)v; }},
    {"r16 Roff=8", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.res = ptr(0x40000); p.ldres = 512; p.res_dtype = VMC_BF16; p.res = ptr(0x40000 + 8); (void)p; (void)v; }},
    {"boff=4", VMC_E_ALIGN, [](GemmProblem& p, int& v) { p.bias = ptr(0x50000 + 4); (void)p; (void)v; }},
    {"lda=512", VMC_E_ARG, [](GemmProblem& p, int& v) { p.lda = 512; (void)p; (void)v; }},
    {"ldw=960", VMC_E_ARG, [](GemmProblem& p, int& v) { p.ldw = 960; (void)p; (void)v; }},
    {"ldc=256", VMC_E_ARG, [](GemmProblem& p, int& v) { p.ldc = 256; (void)p; (void)v; }},
    {"od=3", VMC_E_DTYPE, [](GemmProblem& p, int& v) { p.out_dtype = 3; (void)p; (void)v; }},
    {"od=2", VMC_E_DTYPE, [](GemmProblem& p, int& v) { p.out_dtype = 2; (void)p; (void)v; }},
    {"r16 rd=2", VMC_E_DTYPE, [](GemmProblem& p, int& v) { p.res = ptr(0x40000); p.ldres = 512; p.res_dtype = VMC_BF16; p.res_dtype = 2; (void)p; (void)v; }},
    {"act=4", VMC_E_ARG, [](GemmProblem& p, int& v) { p.act = 4; (void)p; (void)v; }},
    {"act=-1", VMC_E_ARG, [](GemmProblem& p, int& v) { p.act = -1; (void)p; (void)v; }},
    {"(valid)", 0, [](GemmProblem& p, int& v) {  (void)p; (void)v; }},
};

struct TnCase {
  const char* name;
  int M, N, K, lddy, ldx;
  const char* ov;
  const char* want;
  size_t workspace;
};
static const TnCase kTnCases[] = {
    {"student qkv", 25600, 2304, 768, 2304, 768, "", "tn256 s=9 p=23", 63783936u},
    {"student qkv tn256=0", 25600, 2304, 768, 2304, 768, "tn256=0", "tn s=4", 63783936u},
    {"student out_proj", 25600, 768, 768, 768, 768, "", "tn s=14", 33073152u},
    {"student out_proj tn256=0", 25600, 768, 768, 768, 768, "tn256=0", "tn s=14", 33073152u},
    {"student c_fc", 25600, 3072, 768, 3072, 768, "", "tn256 s=7 p=29", 66146304u},
    {"student c_fc tn256=0", 25600, 3072, 768, 3072, 768, "tn256=0", "tn s=3", 66146304u},
    {"student c_proj", 25600, 768, 3072, 768, 3072, "", "tn256 s=7 p=29", 66081792u},
    {"student c_proj tn256=0", 25600, 768, 3072, 768, 3072, "tn256=0", "tn s=3", 66081792u},
    {"tfam B=512 D=512 qkv", 8192, 1536, 512, 1536, 512, "", "tn s=10", 31518720u},
    {"tfam B=512 D=512 out", 8192, 512, 512, 512, 512, "", "tn s=32", 33619968u},
    {"tfam B=512 D=512 ff1", 8192, 2048, 512, 2048, 512, "", "tn s=8", 33619968u},
    {"tfam B=512 D=512 ff2", 8192, 512, 2048, 512, 2048, "", "tn s=8", 33570816u},
    {"tfam B=512 D=512 cls", 8192, 256, 512, 256, 512, "", "tn s=32", 16809984u},
    {"tfam B=512 D=512 head", 8192, 144, 256, 144, 256, "", "tn s=32", 4737024u},
    {"tfam B=512 D=768 qkv", 8192, 2304, 768, 2304, 768, "", "tn256 s=8 p=8", 56696832u},
    {"tfam B=512 D=768 out", 8192, 768, 768, 768, 768, "", "tn s=13", 30710784u},
    {"tfam B=512 D=768 ff1", 8192, 2048, 768, 2048, 768, "", "tn s=5", 31498240u},
    {"tfam B=512 D=768 ff2", 8192, 768, 2048, 768, 2048, "", "tn s=5", 31472640u},
    {"tfam B=512 D=768 cls", 8192, 384, 768, 384, 768, "", "tn s=19", 22442496u},
    {"tfam B=512 D=768 head", 8192, 144, 384, 144, 384, "", "tn s=32", 7096320u},
    {"student qkv minpairs=24", 25600, 2304, 768, 2304, 768, "tn256_min_pairs=24", "tn s=4", 28348416u},
    {"student qkv minpairs=23", 25600, 2304, 768, 2304, 768, "tn256_min_pairs=23", "tn256 s=9 p=23", 63783936u},
    {"tfam ff1 minpairs=4", 8192, 2048, 512, 2048, 512, "tn256_min_pairs=4", "tn256 s=16 p=4", 67239936u},
    {"vitl c_fc wgrad", 65792, 4096, 1024, 4096, 1024, "", "tn256 s=4 p=129", 67174400u},
    {"vitl qkv wgrad strided", 65792, 3072, 1024, 4096, 1024, "", "tn256 s=5 p=103", 62976000u},
    {"token tail", 25608, 768, 768, 768, 768, "", "tn s=14", 33073152u},
    {"operand >= 2 GiB", 1048576, 1024, 768, 1024, 768, "", "tn s=10", 31498240u},
};

struct SplitKCase {
  int M, N, K, slices;
  size_t workspace;
};
static const SplitKCase kSplitKCases[] = {     // ops.linear_wgrad: tiles of 128^2 < 384 and K >= 1024
    {768, 768, 25600, 22, 51904512u},
    {3072, 768, 25600, 6, 56623104u},
    {768, 3072, 25600, 6, 56623104u},
    {512, 2048, 8192, 12, 50331648u},
    {140, 384, 8192, 32, 6881280u},
    {256, 512, 1024, 4, 2097152u},
    {1024, 1024, 65792, 12, 50331648u},
    {768, 768, 1024, 4, 9437184u},
    {2048, 2048, 1024, 3, 50331648u},
};

int main() {
  for (const GemmCase& c : kGemmCases) {
    const GemmProblem p = prob(c.M, c.N, c.K, c.flags);
    CHECK(gemm_check(p, c.variant) == 0, "%s: rejected", c.name);
    const GemmPlan pl = gemm_route(p, c.variant, overrides(c.ov));
    const std::string got = plan_str(pl);
    CHECK(got == c.want, "%s (variant %d, %s): %s, want %s", c.name, c.variant, c.ov, got.c_str(), c.want);
    check_plan(c.name, p, pl);
  }
  for (const ErrCase& c : kErrCases) {
    GemmProblem p = prob(1024, 512, 1024, "b");
    int variant = VMC_GEMM_DEFAULT;
    c.bad(p, variant);
    CHECK(gemm_check(p, variant) == c.want, "%s: %d, want %d", c.what, gemm_check(p, variant), c.want);
  }
  for (const TnCase& c : kTnCases) {
    const GemmOverrides ov = overrides(c.ov);
    const TnPlan t = tn_route(c.M, c.N, c.K, c.lddy, c.ldx, ov);
    char got[64];
    if (t.k256) snprintf(got, sizeof got, "tn256 s=%d p=%d", t.slices, t.pairs_per_slice);
    else snprintf(got, sizeof got, "tn s=%d", t.slices);
    CHECK(!strcmp(got, c.want), "%s: %s, want %s", c.name, got, c.want);
    CHECK(tn_workspace_bytes(c.M, c.N, c.K, ov) == c.workspace, "%s: workspace %zu, want %zu", c.name, tn_workspace_bytes(c.M, c.N, c.K, ov), c.workspace);
    CHECK(tn_slab_bytes(t.slices, c.N, c.K) <= c.workspace, "%s: slabs exceed the workspace", c.name);
    if (t.k256) CHECK(c.M / 128 <= t.slices * t.pairs_per_slice && c.M / 128 > (t.slices - 1) * t.pairs_per_slice, "%s: empty or missing slice", c.name);
  }
  const GemmTileCfg& sk = kGemmTileCfgs[kGemmSplitKCfg];
  CHECK(sk.ks == 1 && sk.u == 1 && !sk.none_only, "split-K tile: no K-slice groups, one K tile per barrier");
  for (const SplitKCase& c : kSplitKCases) {
    CHECK(splitk_slices(c.M, c.N, c.K) == c.slices, "split-K %dx%dx%d: %d slices, want %d", c.M, c.N, c.K, splitk_slices(c.M, c.N, c.K), c.slices);
    CHECK(splitk_workspace_bytes(c.M, c.N, c.K) == c.workspace, "split-K %dx%dx%d: workspace %zu, want %zu", c.M, c.N, c.K,
          splitk_workspace_bytes(c.M, c.N, c.K), c.workspace);
  }
  // every switch keeps its name and default
  static const char* const kEnv[] = {"VMC_GEMM_CFG", "VMC_GEMM_KS", "VMC_GEMM_U", "VMC_GEMM_MFMA32", "VMC_GEMM_GC", "VMC_TN256", "VMC_TN256_MINPAIRS"};
  for (const char* e : kEnv) unsetenv(e);
  GemmOverrides o = gemm_overrides_from_env();
  CHECK(o.cfg == 0 && !o.ks && o.u == 4 && !o.mfma32 && o.gc == 0 && o.tn256 && o.tn256_min_pairs == 8, "defaults");
  setenv("VMC_GEMM_CFG", "7", 1); setenv("VMC_GEMM_KS", "1", 1); setenv("VMC_GEMM_U", "2", 1); setenv("VMC_GEMM_MFMA32", "1", 1);
  setenv("VMC_GEMM_GC", "3", 1); setenv("VMC_TN256", "0", 1); setenv("VMC_TN256_MINPAIRS", "24", 1);
  o = gemm_overrides_from_env();
  CHECK(o.cfg == 7 && o.ks && o.u == 2 && o.mfma32 && o.gc == 3 && !o.tn256 && o.tn256_min_pairs == 24, "switches from the environment");
  setenv("VMC_GEMM_KS", "0", 1); setenv("VMC_TN256", "1", 1);
  o = gemm_overrides_from_env();
  CHECK(!o.ks && o.tn256, "VMC_GEMM_KS=0 / VMC_TN256=1");

  const int n = (int)(sizeof kGemmCases / sizeof kGemmCases[0] + sizeof kErrCases / sizeof kErrCases[0] + sizeof kTnCases / sizeof kTnCases[0] +
                      sizeof kSplitKCases / sizeof kSplitKCases[0]);
  if (fails) {
    printf("%d FAILED\n", fails);
    return 1;
  }
  printf("OK: %d routing cases\n", n);
  return 0;
}
