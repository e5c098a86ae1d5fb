// GEMM dispatch as pure functions: which kernel instantiation, tile configuration and row range a vmc_linear* call launches,
// which weight-gradient kernel and how many token slices a TN call takes, and the workspace sizes that follow from them.
// No HIP types: the launchers in gemm.hip / gemm8.hip / gemm_tn.hip / gemm_tn256.hip execute these plans, and
// tests/host/test_gemm_route.cpp (plain g++) pins them for the shapes the models issue.  Measurements behind the thresholds:
// DESIGN.md §3.1, §3.3 and profiles/README.md.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vmc.h"

// ---- instantiated kernels ----------------------------------------------------------------------------------------------------
// gemm_kernel<T, ACT, MT, WM, WN, NS, KS, U> (gemm.hip): block tile (16 MT WM) x (64 WN), NS LDS stages (> 2: ring), KS K-slice
// groups, U K tiles per barrier.  `none_only`: the VMC_GEMM_CFG sweep, instantiated for VMC_ACT_NONE only.
struct GemmTileCfg { int mt, wm, wn, ns, ks, u; bool none_only; };
constexpr GemmTileCfg kGemmTileCfgs[] = {
    {8, 2, 4, 2, 1, 1, false},  //  0  256 x 256, two stages
    {4, 2, 2, 2, 1, 1, false},  //  1  128 x 128, two stages (also split-K and VMC_GEMM_CFG=6)
    {2, 2, 1, 4, 1, 1, false},  //  2  64 x 64, 4-stage ring (also VMC_GEMM_CFG=5)
    {2, 2, 1, 8, 1, 4, false},  //  3  ... four K tiles per barrier on an 8-slot ring
    {2, 2, 1, 6, 1, 2, false},  //  4  ... two K tiles per barrier on a 6-slot ring (VMC_GEMM_U=2)
    {2, 2, 1, 4, 2, 1, false},  //  5  ... two K-slice groups (VMC_GEMM_KS=1)
    {1, 2, 1, 4, 1, 1, false},  //  6  32 x 64, 4-stage ring
    {1, 2, 1, 8, 1, 4, false},  //  7  ... four K tiles per barrier
    {1, 2, 1, 6, 1, 2, false},  //  8  ... two K tiles per barrier (VMC_GEMM_U=2)
    {1, 2, 1, 3, 4, 1, false},  //  9  ... four K-slice groups on 3-stage rings (VMC_GEMM_KS=1)
    {4, 2, 2, 3, 1, 1, true},   // 10  VMC_GEMM_CFG=1   128 x 128, 3-stage ring
    {4, 2, 2, 4, 1, 1, true},   // 11  VMC_GEMM_CFG=2   128 x 128, 4-stage ring
    {4, 2, 1, 4, 1, 1, true},   // 12  VMC_GEMM_CFG=3   128 x 64, 4-stage ring
    {2, 2, 2, 4, 1, 1, true},   // 13  VMC_GEMM_CFG=4   64 x 128, 4-stage ring
    {4, 2, 1, 6, 1, 1, true},   // 14  VMC_GEMM_CFG=7   128 x 64, 6-stage ring
    {2, 2, 2, 6, 1, 1, true},   // 15  VMC_GEMM_CFG=8   64 x 128, 6-stage ring
    {8, 2, 2, 2, 1, 1, true},   // 16  VMC_GEMM_CFG=9   256 x 128, two stages
    {8, 2, 2, 3, 1, 1, true},   // 17  VMC_GEMM_CFG=10  256 x 128, 3-stage ring
    {4, 2, 4, 2, 1, 1, true},   // 18  VMC_GEMM_CFG=11  128 x 256, two stages
};
constexpr int kGemmTileCfgCount = sizeof(kGemmTileCfgs) / sizeof(kGemmTileCfgs[0]);
constexpr int kGemmCfgSweep[12] = {-1, 10, 11, 12, 13, 2, 1, 14, 15, 16, 17, 18};   // VMC_GEMM_CFG value -> entry
enum { GEMM_T256 = 0, GEMM_T128 = 1, GEMM_T64 = 2, GEMM_T32 = 6 };   // the routed groups: +1 U = 4, +2 U = 2, +3 K-slice groups
constexpr int kGemmSplitKCfg = GEMM_T128;

// gemm8p_kernel / gemm8p32_kernel<T, ACT, BIAS, ZOUT> (gemm8.hip): the persistent walks, each a ~2000-instruction kernel, so only
// these epilogues exist.  erf-GELU spills in the persistent kernel (scratch accesses count in vmcnt) and has none.
struct Gemm8pInst { int act; bool bias, zout, mfma32; };
constexpr Gemm8pInst kGemm8pInsts[] = {
    {VMC_ACT_NONE, true, false, false},     {VMC_ACT_NONE, false, false, false}, {VMC_ACT_QUICKGELU, true, false, false},
    {VMC_ACT_QUICKGELU, true, true, false}, {VMC_ACT_RELU, true, false, false},  {VMC_ACT_NONE, true, false, true},
    {VMC_ACT_NONE, false, false, true},     {VMC_ACT_QUICKGELU, true, false, true}};
constexpr int kGemm8pInstCount = sizeof(kGemm8pInsts) / sizeof(kGemm8pInsts[0]);

// ---- the builder's A/B switches (environment; read once per process, at the first GEMM call) ----------------------------------
struct GemmOverrides {
  int cfg = 0;               // VMC_GEMM_CFG: 1..11 force a tile (kGemmCfgSweep) on the small-tile path of VMC_ACT_NONE calls
  bool ks = false;           // VMC_GEMM_KS: K-slice groups on the long-K small problems (not bit-identical to the persistent kernel)
  int u = 4;                 // VMC_GEMM_U: K tiles per barrier of the small-tile rings (4 or 2; anything else: 1)
  bool mfma32 = false;       // VMC_GEMM_MFMA32: the persistent walk on 32x32x16 fragments wherever instantiated
  int gc = 0;                // VMC_GEMM_GC: column panels per tile-walk group of gemm8 (0 = 4)
  bool tn256 = true;         // VMC_TN256=0: weight gradients never take the 256 x 256 TN kernel
  int tn256_min_pairs = 8;   // VMC_TN256_MINPAIRS: fewest 128-token pairs per slice the 256 x 256 TN kernel takes
};
inline GemmOverrides gemm_overrides_from_env() {
  auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  return {env("VMC_GEMM_CFG", 0), env("VMC_GEMM_KS", 0) != 0, env("VMC_GEMM_U", 4), env("VMC_GEMM_MFMA32", 0) != 0, env("VMC_GEMM_GC", 0),
          env("VMC_TN256", 1) != 0, env("VMC_TN256_MINPAIRS", 8)};
}
inline const GemmOverrides& gemm_overrides() {
  static const GemmOverrides o = gemm_overrides_from_env();
  return o;
}

// ---- vmc_linear / vmc_linear_variant / vmc_linear_preact ----------------------------------------------------------------------
struct GemmProblem {      // one call, as passed (pointers only checked and offset, never dereferenced here)
  const void *A, *W, *bias, *res, *C, *Z;
  int M, N, K, lda, ldw, ldc, ldres, ldz, act;
  float alpha;
  int out_dtype, res_dtype, out_row_group, res_row_mod, dtype16;
};
enum { GEMM_TILE = 0, GEMM_8 = 1, GEMM_8P = 2 };   // gemm_kernel, gemm8_kernel (one tile per workgroup), the persistent walks
// cfg: kGemmTileCfgs entry (GEMM_TILE), kGemm8pInsts entry (GEMM_8P), 0 (GEMM_8); the launch covers rows [row0, row0 + rows)
struct GemmLaunch { int family, cfg, row0, rows; };
struct GemmPlan { int n; GemmLaunch launch[2]; };   // n = 2: the tail split

inline int gemm_check(const GemmProblem& p, int variant) {
  if (variant < 0 || variant >= VMC_GEMM_VARIANTS) return VMC_E_ARG;
  if (!p.A || !p.W || !p.C || p.M <= 0 || p.N <= 0 || p.K <= 0) return VMC_E_ARG;
  if (p.Z && (p.ldz < p.N || (p.ldz % 4) || ((uintptr_t)p.Z & 15) || p.out_row_group)) return VMC_E_ARG;
  if (p.dtype16 != VMC_BF16 && p.dtype16 != VMC_F16) return VMC_E_DTYPE;
  if (p.K % 64 != 0 || p.N % 4 != 0) return VMC_E_SHAPE;
  if (p.lda % 8 || p.ldw % 8 || p.ldc % 4 || (p.res && (p.ldres % 4))) return VMC_E_ALIGN;
  if (((uintptr_t)p.A | (uintptr_t)p.W | (uintptr_t)p.C | (uintptr_t)p.res | (uintptr_t)p.bias) & 15) return VMC_E_ALIGN;
  if (p.lda < p.K || p.ldw < p.K || p.ldc < p.N) return VMC_E_ARG;
  if (p.out_dtype != VMC_F32 && p.out_dtype != p.dtype16) return VMC_E_DTYPE;
  if (p.res && p.res_dtype != VMC_F32 && p.res_dtype != p.dtype16) return VMC_E_DTYPE;
  if (p.act < VMC_ACT_NONE || p.act > VMC_ACT_RELU) return VMC_E_ARG;
  return 0;
}

// Small-tile configuration for M rows (k_slices == 1).  The 256x256 tile needs >= ~1 tile per CU to pay; smaller problems take
// smaller tiles so the grid still covers the 256 CUs.  64x64 tiles are latency-bound, hence the rings; a workgroup streams its
// (BM + 64) x K operand bytes at the ~70 GB/s one CU pulls from L2, so a long K chain on at most 128 workgroups of 64^2 takes 32-row
// tiles (twice the CUs, same per-row arithmetic and K order: same bits).  U K tiles per barrier keep the K order (same bits); an
// 8-slot ring of 64^2 tiles is 128 KiB, one workgroup per CU, so only problems of at most one workgroup per CU take it.  K-slice
// groups sum the K tiles in another order than the persistent kernel, so they are not routed by default (VMC_GEMM_KS=1): a row's
// bits would depend on whether it falls into a GEMM's 256-row tail.
inline int gemm_tile_cfg(int M, int N, int K, int act, const GemmOverrides& ov) {
  if (act == VMC_ACT_NONE && ov.cfg >= 1 && ov.cfg <= 11) return kGemmCfgSweep[ov.cfg];
  const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64);
  if (t256 >= 192) return GEMM_T256;
  if (t128 >= 128) return GEMM_T128;
  const int base = t64 <= 128 && K >= 1024 ? GEMM_T32 : GEMM_T64;
  const bool u_ok = K >= 512 && t64 <= 256;
  if (ov.ks && K >= 1024 && t64 <= 256) return base + 3;
  if (ov.u == 2 && u_ok && (K / 64) % 2 == 0) return base + 2;
  if (ov.u == 4 && u_ok && (K / 64) % 4 == 0) return base + 1;
  return base;
}

// The 8-phase 256x256 kernels on rows [0, rows).  The persistent walk takes problems made of whole 256x256 tiles (at least 192 of
// them, at least two K iterations) with a plain 16-bit output (gemm8.hip's G8_EPI_STORE16) and an instantiated epilogue;
// everything else runs one tile per workgroup.
inline GemmLaunch gemm8_launch(const GemmProblem& p, int rows, int variant, const GemmOverrides& ov) {
  const bool whole = !(rows & 255) && !(p.N & 255) && (long)(rows / 256) * (p.N / 256) >= 192 && p.K >= 256;
  const bool offsets32 = (size_t)rows * p.lda * 2 < (1ull << 31) && (size_t)p.N * p.ldw * 2 < (1ull << 31) &&   // buffer descriptors
                         (size_t)255 * p.ldc * 2 + 512 < (1ull << 31) && (!p.Z || p.ldz == p.ldc);
  const bool store16 = !(p.ldc & 7) && !p.out_row_group && p.out_dtype != VMC_F32 && !p.res && (!p.Z || !(p.ldz & 7));
  if (variant != VMC_GEMM_ONE_TILE && whole && offsets32 && store16) {
    const bool want32 = ov.mfma32 || variant == VMC_GEMM_MFMA32;
    for (int pass = want32 ? 0 : 1; pass < 2; ++pass)      // the 32x32 walk first where asked for, then the 16x16 one
      for (int i = 0; i < kGemm8pInstCount; ++i) {
        const Gemm8pInst& k = kGemm8pInsts[i];
        if (k.mfma32 == (pass == 0) && k.act == p.act && k.bias == (p.bias != nullptr) && k.zout == (p.Z != nullptr))
          return {GEMM_8P, i, 0, rows};
      }
  }
  return {GEMM_8, 0, 0, rows};
}

inline GemmPlan gemm_route(const GemmProblem& p, int variant, const GemmOverrides& ov) {
  const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
  const long t128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
  // Between 129 and 191 tiles of 256x256 the 128x128 kernel would need a second round of its 512 resident workgroups (t128 > 512)
  // while the 8-phase kernel still finishes in one: M = 4096, N = 2304, K = 768 (TFAM qkv at 256 clips) 31.6 -> 21.2 us; at <= 128
  // tiles the two are equal (20.8 / 20.0 us at 96 tiles) and below 96 the small tiles win.  The 8-phase kernels take K tile pairs.
  const bool big = t256 >= 192 || (t256 > 128 && t128 > 512);
  if (variant == VMC_GEMM_TWOSTAGE || !big || p.K % 128 != 0) return {1, {{GEMM_TILE, gemm_tile_cfg(p.M, p.N, p.K, p.act, ov), 0, p.M}}};
  // Round quantisation: T tiles on 256 CUs cost ceil(T/256) tile-times.  When the last, partial round holds only a few tiles
  // (ViT-L/14: 257 x tn tiles -> tn tiles in a round of their own: +25 % at tn = 4; student ViT-B/32: 100 x 3 tiles -> 44 tiles in a
  // second round), the tile rows that do not fit the full rounds go to the small-tile kernels, which spread them over the whole
  // chip, in a second launch.  Whole tile rows fit the full rounds (a last main round may leave up to tn - 1 CUs idle).
  const int tm = (p.M + 255) / 256, tn = (p.N + 255) / 256;
  const int rounds = (int)(t256 / 256);
  const int main_rows = rounds > 0 ? (rounds * 256) / tn : 0;
  const long tail = (long)(tm - main_rows) * tn;
  if (variant != VMC_GEMM_NO_TAIL_SPLIT && !p.out_row_group && !p.res_row_mod && main_rows > 0 && main_rows < tm && t256 % 256 != 0 &&
      tail <= (rounds >= 2 ? 64 : 96)) {
    const int m_main = main_rows * 256;
    return {2, {gemm8_launch(p, m_main, variant, ov), {GEMM_TILE, gemm_tile_cfg(p.M - m_main, p.N, p.K, p.act, ov), m_main, p.M - m_main}}};
  }
  return {1, {gemm8_launch(p, p.M, variant, ov)}};
}

// ---- vmc_linear_splitk_f32: 128x128 tiles (kGemmSplitKCfg) x K slices, partial slabs + a fixed-order reduce ---------------------
inline int splitk_slices(int M, int N, int K) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int slices = (768 + tiles - 1) / tiles;              // ~3 workgroups per CU
  const int nkt = K / 64;
  if (slices > nkt / 4) slices = nkt / 4;              // at least 4 K tiles per slice
  if (slices < 1) slices = 1;
  const int per = (nkt + slices - 1) / slices;         // the kernel's per-slice tile count ...
  return (nkt + per - 1) / per;                        // ... and no empty trailing slice (its slab would stay unwritten)
}
inline size_t splitk_workspace_bytes(int M, int N, int K) {
  const int s = splitk_slices(M, N, K);
  return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;
}

// ---- vmc_linear_wgrad_tn / vmc_linear_wgrad_bias_tn: C[N,K] = dY[M,N]^T X[M,K], token slices + a fixed-order reduce ------------
// k256: the 256 x 256 tile (gemm_tn256.hip), else 256 x 128 (gemm_tn.hip); pairs_per_slice: 128-token pairs (256 x 256 only)
struct TnPlan { bool k256; int slices, pairs_per_slice; };
// 256 x 128 kernel, one workgroup per CU (144 KiB of LDS): aim at whole rounds of 256 workgroups -- one round when the tiles allow
// it (fewer, longer slices: half the slab traffic of the reduce), two when a single round would leave > 1/4 of the chip idle
// (measured against ceil(512 / tiles) slices: 62 vs 83 us at 768x768, 164 vs 206 us at 3072x768, M = 25 600)
inline int tn_slices(int M, int N, int K) {
  const int tiles = ((N + 255) / 256) * ((K + 127) / 128);
  int slices = 256 / tiles;
  if (slices >= 1 && tiles * slices < 192) slices = 512 / tiles;
  const int steps = (M + 63) / 64;
  if (slices > steps / 4) slices = steps / 4;
  if (slices < 1) slices = 1;
  const int per = (steps + slices - 1) / slices;
  return (steps + per - 1) / per;                      // no empty trailing slice
}
// 256 x 256 kernel, one workgroup per CU (128 KiB of LDS): one round of at most 256 workgroups
inline TnPlan tn256_plan(int M, int N, int K) {
  const int tiles = ((N + 255) / 256) * ((K + 255) / 256), pairs = M / 128;
  int s = 256 / tiles;
  if (s > pairs / 2) s = pairs / 2;
  if (s < 1) s = 1;
  const int per = (pairs + s - 1) / s;
  return {true, (pairs + per - 1) / per, per};         // no empty trailing slice
}
// Large problems made of whole 128-token pairs take the 256 x 256 tile.  Fewer than 16 tiles: too many slabs for the reduce
// (768 x 768: 28); short slices are all prologue and slab traffic (M = 4096, 512 x 2048: 16 slices of two pairs, 32 vs 27 us).
inline TnPlan tn_route(int M, int N, int K, int lddy, int ldx, const GemmOverrides& ov) {
  if (ov.tn256 && M >= 256 && !(M & 127) && (long)((N + 255) / 256) * ((K + 255) / 256) >= 16 &&
      (size_t)M * lddy * 2 < (1ull << 31) && (size_t)M * ldx * 2 < (1ull << 31)) {      // buffer descriptors
    const TnPlan p = tn256_plan(M, N, K);
    if (p.pairs_per_slice >= ov.tn256_min_pairs) return p;
  }
  return {false, tn_slices(M, N, K), 0};
}
inline size_t tn_slab_bytes(int slices, int N, int K) {          // weight slabs, then bias slabs
  return slices > 1 ? (size_t)slices * ((size_t)N * K + N) * sizeof(float) : 0;
}
// The leading dimensions are not known here: room for whichever kernel the call takes, VMC_TN256 or not.
inline size_t tn_workspace_bytes(int M, int N, int K, GemmOverrides ov) {
  ov.tn256 = true;
  const int s = tn_route(M, N, K, N, K, ov).slices, s128 = tn_slices(M, N, K);
  return tn_slab_bytes(s > s128 ? s : s128, N, K);
}
