// Attention dispatch as pure functions: which kernel instantiation a vmc_attention_vit_fwd / vmc_attention_vit_cls_fwd /
// vmc_attention_fwd / vmc_attention_bwd call launches, with which grid, block, dynamic LDS and row stride, or which error code it
// returns instead, with the arguments checked in a fixed order.  No HIP types: the executors in attention.hip / attention_long.hip /
// attention_vit_long.hip launch these plans, and tests/host/test_attn_route.cpp (plain g++) pins them.  The functions are static
// inline, so none of them becomes a symbol of libvmc.so.  The kernels: DESIGN.md §3.2 (ViT, in LDS and streamed) and §3.7 (masked,
// any length).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vmc.h"

// ---- constants the kernels and the route share ------------------------------------------------------------------------------
constexpr int ATT_MAX_TK = 2048;                 // the scalar kernels keep a score row of ATT_MAX_TK floats in LDS ...
constexpr int ATT_MAX_DH = 128;                  // ... and query / key rows of ATT_MAX_DH floats
constexpr int ATT_BWD_MAX_LDS = 160 * 1024;      // attn_bwd_mfma_kernel: Q, dO, K, V of a head, lse and delta
constexpr int ATT_VIT_MAX_N = 288;               // attn_vit_kernel: a head's K / V in LDS, at most 18 16-key tiles
constexpr int ATT_LONG_LT = 64;                  // attention_long.hip: rows of every tile (queries per workgroup, keys per tile)
constexpr int ATT_LONG_NTH = 256;                // ... threads per workgroup of every tiled kernel
constexpr int ATT_VL_KT = 64;                    // attention_vit_long.hip: keys per K / V tile
constexpr int ATT_VL_NW = 4;                     // ... waves per workgroup (both kernels)
constexpr int ATT_VL_QROWS = ATT_VL_NW * 32;     // ... query rows per workgroup of the full kernel
constexpr int ATT_VL_NC = 577;                   // ... the key count instantiated at compile time (ViT-L/14@336px)
constexpr int ATT_VL_CLS_LDS = ATT_VL_NW * 2 * 2 * ATT_VL_KT * 128;   // class query: K | V images of two tiles per wave (128 KB)

// ---- instantiated kernels (each for BF16 and F16) ---------------------------------------------------------------------------
enum AttnKernel {
  ATTN_VIT,             // attn_vit_kernel<T, NT, NC, NW, REREAD, PERSIST>: a kAttnVitInsts entry
  ATTN_VIT_LONG,        // attn_vit_long_kernel<T, NC>
  ATTN_VIT_LONG_CLS,    // attn_vit_long_cls_kernel<T, NC>
  ATTN_SMALL,           // attn_small_kernel<T, DH, NT>
  ATTN_LONG_FWD,        // attn_long_fwd_kernel<T, DH>
  ATTN_GENERIC_FWD,     // attn_generic_fwd<T>
  ATTN_BWD_MFMA,        // attn_bwd_mfma_kernel<T, DH>
  ATTN_LONG_BWD,        // attn_long_delta_kernel -> attn_long_bwd_kv_kernel -> attn_long_bwd_q_kernel<T, DH>
  ATTN_GENERIC_BWD,     // attn_generic_bwd_q -> attn_generic_bwd_kv<T>
};

// attn_vit_kernel: NT 16-key tiles in LDS, key count NC (0: runtime N), NW waves (64 NW threads), K fragments re-read per query
// tile (REREAD), persistent walk over (frame, head) pairs (PERSIST).  The default at N = 257 (112 VGPRs, 4 waves per SIMD) takes
// 167-169 us per ViT-L/14 layer against 171-174 us for the 4-wave kernel (252 VGPRs); the persistent walks measured slower or
// equal (profiles/README.md).
struct AttnVitInst { int nt, nc, nw; bool reread, persist; };
constexpr AttnVitInst kAttnVitInsts[] = {
    {18, 257, 8, true, false},    //  0  N = 257 full call, the default (VMC_ATTN_VARIANT=1)
    {18, 257, 4, true, false},    //  1  VMC_ATTN_VARIANT=2
    {18, 257, 4, false, true},    //  2  VMC_ATTN_VARIANT=10..19: stagger variant - 10
    {18, 257, 8, true, true},     //  3  VMC_ATTN_VARIANT=20..29: stagger variant - 20
    {18, 257, 4, false, false},   //  4  any other variant (9: the 4-wave kernel of round 2), and the class query at N = 257
    {14, 197, 4, false, false},   //  5  ViT-B/16
    {4, 50, 4, false, false},     //  6  ViT-B/32
    {2, 0, 4, false, false},      //  7  N <= 32
    {4, 0, 4, false, false},      //  8  N <= 64
    {8, 0, 4, false, false},      //  9  N <= 128
    {14, 0, 4, false, false},     // 10  N <= 224
    {18, 0, 4, false, false},     // 11  N <= 288
};
constexpr int kAttnVitInstCount = sizeof(kAttnVitInsts) / sizeof(kAttnVitInsts[0]);

// The other instantiations with their __launch_bounds__ (threads per block); template arguments a kernel does not take are 0.
struct AttnInst { int kernel, dh, nt, nc, bound; };
constexpr AttnInst kAttnInsts[] = {
    {ATTN_VIT_LONG, 0, 0, ATT_VL_NC, 64 * ATT_VL_NW},     {ATTN_VIT_LONG, 0, 0, 0, 64 * ATT_VL_NW},
    {ATTN_VIT_LONG_CLS, 0, 0, ATT_VL_NC, 64 * ATT_VL_NW}, {ATTN_VIT_LONG_CLS, 0, 0, 0, 64 * ATT_VL_NW},
    {ATTN_SMALL, 64, 2, 0, 64},   {ATTN_SMALL, 64, 4, 0, 64},   {ATTN_SMALL, 96, 2, 0, 64},   {ATTN_SMALL, 96, 4, 0, 64},
    {ATTN_LONG_FWD, 64, 0, 0, ATT_LONG_NTH},  {ATTN_LONG_FWD, 96, 0, 0, ATT_LONG_NTH},  {ATTN_GENERIC_FWD, 0, 0, 0, 64},
    {ATTN_BWD_MFMA, 64, 0, 0, 256},           {ATTN_BWD_MFMA, 96, 0, 0, 256},
    {ATTN_LONG_BWD, 64, 0, 0, ATT_LONG_NTH},  {ATTN_LONG_BWD, 96, 0, 0, ATT_LONG_NTH},  {ATTN_GENERIC_BWD, 0, 0, 0, 64},
};
constexpr int kAttnInstCount = sizeof(kAttnInsts) / sizeof(kAttnInsts[0]);

// ---- the builder's A/B switch (environment; attention.hip reads it once per process) ----------------------------------------
struct AttnOverrides {
  int variant = 1;      // VMC_ATTN_VARIANT: the kernel of the N = 257 full call (kAttnVitInsts 0..4; measured: profiles/README.md)
};
static inline AttnOverrides attn_overrides_from_env() {
  const char* v = getenv("VMC_ATTN_VARIANT");
  return {v ? atoi(v) : 1};
}

// ---- one call's arguments as passed (pointers are only tested, never dereferenced here) and its plan -------------------------
// ViT full call: q = qkv, k = qkv + D, v = qkv + 2D, ldq = ldkv = 3D, NQ = N.  Class query: q = q_cls, k = kv, v = kv + D,
// ldq = D, ldkv = 2D, NQ = 1, no lse.
struct AttnVitProblem {
  const void *q, *k, *v;
  void* out;
  float* lse;
  size_t ldq, ldkv;
  int F, N, NQ, H, dtype16;
};
struct AttnFwdProblem {
  const void *q, *k, *v;
  const uint8_t* mask;
  void* out;
  float* lse;
  int B, H, Tq, Tk, dh, ldq, ldk, ldv, ldo;
  float dropout_p;
  uint64_t seed;
  int dtype16;
};
struct AttnBwdProblem {
  const void *q, *k, *v;
  const uint8_t* mask;
  const void *out, *dout;
  const float* lse;
  void *dq, *dk, *dv;
  int B, H, Tq, Tk, dh, ldq, ldk, ldv, ldo, lddq, lddk, lddv;
  float dropout_p;
  uint64_t seed;
  void* workspace;
  size_t workspace_bytes;
  int dtype16;
};

struct AttnPlan {
  int rc = 0;                     // a VMC error code; 0: the fields below are the launch
  int kernel = 0;                 // AttnKernel
  int vit = 0;                    // ATTN_VIT: the kAttnVitInsts entry
  int dh = 0, nt = 0, nc = 0;     // DH of the masked MFMA kernels, NT of attn_small_kernel, NC of the streamed ViT kernels
  unsigned grid[3] = {0, 0, 0};   // ATTN_LONG_BWD: the delta, dK / dV and dQ passes; ATTN_GENERIC_BWD: dQ, dK / dV
  int block = 0;                  // threads per workgroup
  int lds = 0;                    // dynamic LDS bytes
  int rs = 0;                     // ATTN_BWD_MFMA: row stride of the LDS images
  int stagger = 0;                // ATTN_VIT persistent walks: sleeps of the second resident workgroup
};
static inline AttnPlan attn_error(int rc) {
  AttnPlan p;
  p.rc = rc;
  return p;
}
static inline AttnPlan attn_plan(int kernel, size_t grid, int block, int lds = 0) {
  AttnPlan p;
  p.kernel = kernel;
  p.grid[0] = (unsigned)grid;
  p.block = block;
  p.lds = lds;
  return p;
}
static inline bool attn_dtype_ok(int dtype16) { return dtype16 == VMC_BF16 || dtype16 == VMC_F16; }

// ---- vmc_attention_vit_fwd / vmc_attention_vit_cls_fwd ----------------------------------------------------------------------
// N <= 288: attn_vit_kernel, one workgroup per (frame, head) with the head's K / V in LDS; the three CLIP geometries (50 / 197 / 257
// tokens) have their key count compiled in.  Longer: attention_vit_long.hip streams K / V (full call: 128 query rows per
// workgroup; class query: one wave per (frame, head)).  v lies a multiple of 16 bytes past k, so its alignment is k's.
static inline AttnPlan attn_vit_route(const AttnVitProblem& p, const AttnOverrides& ov) {
  if (!p.q || !p.k || !p.out || p.F <= 0 || p.N <= 0 || p.H <= 0) return attn_error(VMC_E_ARG);
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.out) & 15) return attn_error(VMC_E_ALIGN);
  if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
  const int N = p.N;
  if (N <= ATT_VIT_MAX_N) {
    int vit = 4, stagger = 0;                                     // N = 257 unless the full call takes a variant below
    if (N == 257 && p.NQ == N) {                                  // ViT-L/14 @ 224
      const int v = ov.variant;
      vit = v == 1 ? 0 : v == 2 ? 1 : v >= 10 && v < 20 ? 2 : v >= 20 && v < 30 ? 3 : 4;
      stagger = vit == 2 ? v - 10 : vit == 3 ? v - 20 : 0;
    } else if (N != 257) {
      vit = N == 197 ? 5 : N == 50 ? 6 : N <= 32 ? 7 : N <= 64 ? 8 : N <= 128 ? 9 : N <= 224 ? 10 : 11;
    }
    const AttnVitInst& c = kAttnVitInsts[vit];
    const int n_bh = p.F * p.H;
    AttnPlan pl = attn_plan(ATTN_VIT, c.persist && n_bh >= 512 ? 512 : n_bh, 64 * c.nw, 16 * c.nt * 128 * 2);
    pl.vit = vit;
    pl.stagger = stagger;
    return pl;
  }
  AttnPlan pl;
  if (p.NQ == 1) {
    const size_t n_bh = (size_t)p.F * p.H;
    if (n_bh > 0x7FFFFFFF) return attn_error(VMC_E_SHAPE);
    pl = attn_plan(ATTN_VIT_LONG_CLS, (n_bh + ATT_VL_NW - 1) / ATT_VL_NW, 64 * ATT_VL_NW, ATT_VL_CLS_LDS);
  } else {
    const size_t grid = (size_t)p.F * p.H * ((N + ATT_VL_QROWS - 1) / ATT_VL_QROWS);
    if (grid > 0x7FFFFFFF) return attn_error(VMC_E_SHAPE);
    pl = attn_plan(ATTN_VIT_LONG, grid, 64 * ATT_VL_NW);
  }
  pl.nc = N == ATT_VL_NC ? ATT_VL_NC : 0;
  return pl;
}

// ---- vmc_attention_fwd / vmc_attention_bwd ----------------------------------------------------------------------------------
static inline int attn_check_generic(int B, int H, int Tq, int Tk, int dh, int ldq, int ldk, int ldv, int ldo) {
  if (B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return VMC_E_ARG;
  if (dh <= 0 || dh > ATT_MAX_DH || (dh % 8)) return VMC_E_SHAPE;
  if ((ldq % 8) || (ldk % 8) || (ldv % 8) || (ldo % 8)) return VMC_E_ALIGN;
  return 0;
}

// Forward, head dim 64 / 96: Tk <= 64 attn_small_kernel (one wave per (b, h)); longer, the tiled kernel of attention_long.hip
// when out is 8-byte aligned.  Both store 16-bit results as 8-byte words; ldo % 8 == 0, checked first, keeps the rows aligned.
// Everything else: the scalar kernel, one wave per (b, h, query), Tq, Tk <= ATT_MAX_TK.
static inline AttnPlan attn_fwd_route(const AttnFwdProblem& p) {
  if (!p.q || !p.k || !p.v || !p.out || p.dropout_p < 0.f || p.dropout_p >= 1.f) return attn_error(VMC_E_ARG);
  if (int rc = attn_check_generic(p.B, p.H, p.Tq, p.Tk, p.dh, p.ldq, p.ldk, p.ldv, p.ldo)) return attn_error(rc);
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v) & 15) return attn_error(VMC_E_ALIGN);
  const bool mfma = p.dh == 64 || p.dh == 96;
  if (mfma && p.Tk <= 64) {
    if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
    AttnPlan pl = attn_plan(ATTN_SMALL, p.B * p.H, 64);
    pl.dh = p.dh;
    pl.nt = p.Tk <= 32 ? 2 : 4;
    return pl;
  }
  if (mfma && ((uintptr_t)p.out & 7) == 0) {
    if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
    const size_t grid = (size_t)p.B * p.H * ((p.Tq + ATT_LONG_LT - 1) / ATT_LONG_LT);
    if (grid > 0x7FFFFFFF) return attn_error(VMC_E_SHAPE);
    AttnPlan pl = attn_plan(ATTN_LONG_FWD, grid, ATT_LONG_NTH);
    pl.dh = p.dh;
    return pl;
  }
  if (p.Tk > ATT_MAX_TK || p.Tq > ATT_MAX_TK) return attn_error(VMC_E_SHAPE);
  if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
  return attn_plan(ATTN_GENERIC_FWD, p.B * p.H * p.Tq, 64);
}

static inline size_t attn_bwd_workspace_bytes(int B, int H, int Tq) { return (size_t)B * H * Tq * sizeof(float); }

// attn_bwd_mfma_kernel's dynamic LDS at row stride RS: Q, dO, K, V images of whole 32-row steps, then lse and delta per query row.
static inline size_t attn_bwd_lds_bytes(int Tq, int Tk, int RS) {
  const int TQP = (Tq + 31) & ~31, TKP = (Tk + 31) & ~31;
  return (size_t)2 * (TQP + TKP) * RS + (size_t)2 * TQP * sizeof(float);
}

// Backward, head dim 64 / 96 with lddq, lddk, lddv, ldo % 4 == 0: attn_bwd_mfma_kernel when Q, K, V, dO of a head fit in
// ATT_BWD_MAX_LDS with unpadded rows (rows padded by 16 B when that still fits); longer, the tiled passes of attention_long.hip
// when dq, dk, dv are 8-byte and out 16-byte aligned.  Everything else: the scalar kernels, Tq, Tk <= ATT_MAX_TK.
static inline AttnPlan attn_bwd_route(const AttnBwdProblem& p) {
  if (!p.q || !p.k || !p.v || !p.out || !p.dout || !p.lse || !p.dq || !p.dk || !p.dv || !p.workspace) return attn_error(VMC_E_ARG);
  if (int rc = attn_check_generic(p.B, p.H, p.Tq, p.Tk, p.dh, p.ldq, p.ldk, p.ldv, p.ldo)) return attn_error(rc);
  if (p.workspace_bytes < attn_bwd_workspace_bytes(p.B, p.H, p.Tq)) return attn_error(VMC_E_ARG);
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.dout) & 15) return attn_error(VMC_E_ALIGN);
  if ((p.dh == 64 || p.dh == 96) && ((p.lddq | p.lddk | p.lddv | p.ldo) % 4) == 0) {
    if (attn_bwd_lds_bytes(p.Tq, p.Tk, p.dh * 2) <= ATT_BWD_MAX_LDS) {
      if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
      const int RS = attn_bwd_lds_bytes(p.Tq, p.Tk, p.dh * 2 + 16) <= ATT_BWD_MAX_LDS ? p.dh * 2 + 16 : p.dh * 2;
      // one wave per tile task, at most four: a 16-token clip (one key tile + one query tile) runs as a 2-wave workgroup, which
      // lets five of them share a CU instead of three 4-wave ones with two idle waves each
      const int tasks = (p.Tk + 15) / 16 + (p.Tq + 15) / 16;
      AttnPlan pl = attn_plan(ATTN_BWD_MFMA, p.B * p.H, 64 * (tasks < 4 ? tasks : 4), (int)attn_bwd_lds_bytes(p.Tq, p.Tk, RS));
      pl.dh = p.dh;
      pl.rs = RS;
      return pl;
    }
    if ((((uintptr_t)p.dq | (uintptr_t)p.dk | (uintptr_t)p.dv) & 7) == 0 && ((uintptr_t)p.out & 15) == 0) {
      if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
      const size_t bh = (size_t)p.B * p.H, items = bh * p.Tq;
      const size_t gd = (items * 4 + 255) / 256, gkv = bh * ((p.Tk + ATT_LONG_LT - 1) / ATT_LONG_LT),
                   gq = bh * ((p.Tq + ATT_LONG_LT - 1) / ATT_LONG_LT);
      if (gkv > 0x7FFFFFFF || gq > 0x7FFFFFFF || gd > 0x7FFFFFFF) return attn_error(VMC_E_SHAPE);
      AttnPlan pl = attn_plan(ATTN_LONG_BWD, gd, ATT_LONG_NTH);
      pl.grid[1] = (unsigned)gkv;
      pl.grid[2] = (unsigned)gq;
      pl.dh = p.dh;
      return pl;
    }
  }
  if (p.Tk > ATT_MAX_TK || p.Tq > ATT_MAX_TK) return attn_error(VMC_E_SHAPE);
  if (!attn_dtype_ok(p.dtype16)) return attn_error(VMC_E_DTYPE);
  AttnPlan pl = attn_plan(ATTN_GENERIC_BWD, p.B * p.H * p.Tq, 64);
  pl.grid[1] = (unsigned)(p.B * p.H * p.Tk);
  return pl;
}
