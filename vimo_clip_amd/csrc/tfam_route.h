// Dispatch of the fused TFAM chains (tfam_fused.hip: eval forward; tfam_train.hip: training forward + backward) as pure functions:
// which shapes the chains take (tfam_check), the row-block geometry of a batch (tfam_blocks), the column tile of every GEMM
// (tfam_pick_bn / tfam_pick_bn_pair), the launches of every step with kernel instantiation, grid, block and dynamic LDS
// (tfam_route_*), and the workspace layouts.  No HIP types: the executors in the two .hip files fill the kernel arguments and
// launch these plans, and tests/host/test_tfam_route.cpp (plain g++) pins them.  The functions are static inline, so none of them
// becomes a symbol of libvmc.so.  The kernels: DESIGN.md §3.4 (eval chain) and §3.6 (training chains).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vmc.h"

#if defined(__HIPCC__)
#define TFAM_HD __host__ __device__ __forceinline__
#else
#define TFAM_HD static inline
#endif

// ---- constants the kernels and the route share ------------------------------------------------------------------------------
constexpr int TF_BM = 32;                        // token rows of a GEMM workgroup
constexpr int TF_NTH = 256;                      // threads of the ring kernel
constexpr int TF_NW = 8;                         // waves per workgroup of the single-shot kernels (2 row tiles x 4 K slices)
constexpr int TF_MAX_T = 64;                     // tokens per clip (queries in parts of 32 per row block, up to four key tiles)
constexpr size_t TF_LDS_MAX = 160 * 1024;
constexpr int TF_RING_BN = 16, TF_RING_NST = 3;  // K = dim_feedforward / 3 d_model GEMMs: LDS-DMA ring of NST stages of KC columns
constexpr int TF_RING_KC = 512, TR_RING_KC_ALT = 384;      // ... KC; the training chain's K = 3 x 768 takes 384
constexpr int TR_MAX_ROWS = 256;                 // token rows of a training batch (the grouped weight gradient holds <= 4 token stages)
constexpr int TR_MAX_B = 32;                     // clips of a training batch (MAXB of the head backward)
constexpr int TR_HEAD_LDS_MAX = 60 * 1024;       // head backward 1: 32 rows of dlogits in LDS
constexpr int TR_MAX_PROB = 32, TR_MAX_LN = 12;  // problems of one grouped weight-gradient launch
constexpr int TR_WGRAD_FLUSH = 4;                // ... which takes up to four layers' problems (deferred weight gradients)
constexpr int TR_WGRAD_PROBS = 7, TR_WGRAD_LNS = 3;        // ... at most 7 GEMMs and 3 LayerNorms per layer
constexpr int TR_WGRAD_NTH = 512, TR_WGRAD_LDS = 3 * 48 * 1024;      // ... the TN body's three 48-KiB stages (gemm_tn_body.h)
static_assert(TR_WGRAD_FLUSH * TR_WGRAD_PROBS <= TR_MAX_PROB && TR_WGRAD_FLUSH * TR_WGRAD_LNS <= TR_MAX_LN, "weight-gradient table");

enum { PRO_F32 = 0, PRO_LN = 1, PRO_16 = 2, PRO_ATTN = 3, PRO_LNBWD = 4 };
enum { EPI_ACT16 = 0, EPI_RESID32 = 1, EPI_BIAS32 = 2 };

// Fragment-major q / k buffers (tf_frag_off in tfam_kernels.h): token tiles of 16 per (clip, head) record, and their size.
// Clips of up to 32 tokens keep the two-tile records.
TFAM_HD int tf_ntt(int T) { return T <= 32 ? 2 : (T + 15) >> 4; }
TFAM_HD size_t tf_frag_elems(int clips, int H, int DH, int NTT = 2) { return (size_t)clips * H * NTT * (DH >> 5) * 512; }

struct TfDims {
  int B, T, Tk, D, H, ff, L, C, has_cross;
  int proj = 0;      // feature-concatenation mode: the chain starts at projection_layer (the section at the end of this file)
};

// ---- the builder's A/B switches (environment; read once per process by tfam_train.hip) ---------------------------------------
struct TfamOverrides {
  int bn_ff = 0;      // VMC_TR_BN_FF: column tile of the training chain's LayerNorm-prologue GEMMs with N >= 1024 (0: picked)
  int bn_d = 0;       // VMC_TR_BN_D: ... with N < 1024
};
static inline TfamOverrides tfam_overrides_from_env() {
  const char *f = getenv("VMC_TR_BN_FF"), *d = getenv("VMC_TR_BN_D");
  TfamOverrides ov;
  ov.bn_ff = f ? atoi(f) : 0;
  ov.bn_d = d ? atoi(d) : 0;
  return ov;
}

// ---- row-block geometry of a batch ---------------------------------------------------------------------------------------------
// Row blocks: two whole clips (T <= 16), one clip (T <= 32), or -- longer clips -- uniform 32-row blocks for the row-wise GEMMs and
// (clip, 32-query part) blocks for the two attention launches.  An attention workgroup holds qt query tiles and nkt key tiles of 16
// per clip; its V image has the other clips' keys plus keyrows rows.
struct TfamBlocks {
  int M, Mk, dh;                  // token rows, motion-token rows (0 without cross attention), head dim
  int cpb, parts, rpb;            // clips per row block, query parts per clip (attention launches), rows per row block
  int n_rb, n_rb_attn;            // row blocks of a row-wise launch and of an attention launch
  int ntt_q, ntt_k, ntt_kx;       // token tiles per fragment record: queries / self keys, cross keys
  int qt, nkt, nkt_x;             // query tiles; key tiles of the self and the cross attention
  int vrows, vrows_x;             // V-image rows of the self and the cross attention
};
static inline int tfam_nkt(int Tk) { return Tk > 32 ? 4 : (Tk > 16 ? 2 : 1); }
static inline TfamBlocks tfam_blocks(const TfDims& d) {
  TfamBlocks b;
  b.M = d.B * d.T;
  b.Mk = d.has_cross ? d.B * d.Tk : 0;
  b.dh = d.D / d.H;
  b.cpb = d.T <= 16 ? 2 : 1;
  b.parts = d.T > 32 ? (d.T + 31) / 32 : 1;
  b.rpb = d.T > 32 ? 32 : b.cpb * d.T;
  b.n_rb = (b.M + b.rpb - 1) / b.rpb;
  b.n_rb_attn = b.parts > 1 ? d.B * b.parts : b.n_rb;
  b.ntt_q = b.ntt_k = tf_ntt(d.T);
  b.ntt_kx = tf_ntt(d.Tk);
  b.qt = d.T > 16 ? 2 : 1;
  b.nkt = tfam_nkt(d.T);
  b.nkt_x = tfam_nkt(d.Tk);
  b.vrows = (b.cpb - 1) * d.T + 16 * b.nkt;
  b.vrows_x = (b.cpb - 1) * d.Tk + 16 * b.nkt_x;
  return b;
}

// ---- column tiles ------------------------------------------------------------------------------------------------------------------
// A workgroup's cost is one memory round trip plus (32 A rows + BN W rows) x K bytes at the ~70 GB/s one CU pulls from L2, whatever
// BN is; what BN decides is how many workgroups there are.  Take the narrowest tile (most CUs streaming W) whose grid still fits one
// resident round (2 workgroups per CU while the LDS footprint allows, else 1).  The two chains differ in what they may take:
struct TfamTileRule {
  int cand[4], ncand;       // candidate widths, ascending
  bool ragged;              // N < bn is allowed (one ragged tile); false: only widths that divide N
  bool attn_pick;           // attention launches choose between 16 and 32 by LDS; false: always 16
  bool heavy;               // LayerNorm (backward) prologues re-read 32 fp32 rows (and more) per workgroup: one workgroup per CU, and
                            // the TfamOverrides switches apply to them
  int pair_first;           // paired launch: first candidate tried
  bool pair_lds;            // ... candidates must fit TF_LDS_MAX, and the widest feasible one is kept when no grid fits a round
};
constexpr TfamTileRule kTfamEvalTiles = {{16, 32, 48, 64}, 4, true, true, false, 0, true};
constexpr TfamTileRule kTfamTrainTiles = {{16, 32, 64, 0}, 3, false, false, true, 1, false};      // no BN = 48 training kernel

static inline size_t tfam_lds_bytes(int bn, bool attn, int kd, int nkt, int cpb, int Tk) {
  const size_t v = attn ? (size_t)((cpb - 1) * Tk + 16 * nkt) * kd * 2 + 1024 : 0;      // V image + one LDS-DMA piece of slack
  const size_t w = (size_t)bn * kd * 2;
  if (attn && nkt > 2) return (size_t)TF_BM * kd * 2 + (v > w ? v : w);                 // V and W share a region
  return (size_t)(TF_BM + bn) * kd * 2 + v;
}

// heavy_pro: the launch has a LayerNorm (backward) prologue.  vrows: V-image rows of an attention launch.
static inline int tfam_pick_bn(const TfamTileRule& r, const TfamOverrides& ov, int M, int N, int rpb, int K, bool attn, bool heavy_pro,
                               int vrows = 48) {
  if (attn && !r.attn_pick) return 16;
  const bool heavy = r.heavy && heavy_pro;
  if (heavy) {
    int f = 0;
    if (ov.bn_ff && N >= 1024 && N % ov.bn_ff == 0) f = ov.bn_ff;
    else if (ov.bn_d && N < 1024 && N % ov.bn_d == 0) f = ov.bn_d;
    if (f) return (f == 32 || f == 64) ? f : 16;      // a width without a training kernel runs the 16-column one
  }
  const int n_rb = (M + rpb - 1) / rpb;
  int best = 16;
  for (int i = 0; i < r.ncand; ++i) {
    const int bn = r.cand[i];
    if (N % bn && !(r.ragged && N < bn)) continue;
    if (attn && bn > 32) break;
    if (attn && vrows > 48 && bn > 16) break;      // more than 32 keys: the 16-column kernels (V and W share a region)
    const size_t lds = (attn && vrows > 48) ? (size_t)TF_BM * K * 2 + (size_t)vrows * K * 2 + 1024
                                             : (size_t)(TF_BM + bn) * K * 2 + (attn ? (size_t)vrows * K * 2 + 1024 : 0);
    if (lds > TF_LDS_MAX) break;
    best = bn;
    const int per_cu = (lds <= 80 * 1024 && !heavy) ? 2 : 1;
    if ((long)((N + bn - 1) / bn) * n_rb <= 256L * per_cu) break;
  }
  return best;
}

// Column tile of a paired launch (problem b in 32-row blocks): the narrowest that keeps both problems inside one resident round
// (1 workgroup per CU); 64 when none does.
static inline int tfam_pick_bn_pair(const TfamTileRule& r, int Ma, int Na, int rpba, int Mb, int Nb, int K) {
  int best = 64;
  for (int i = r.pair_first; i < r.ncand; ++i) {
    const int bn = r.cand[i];
    if ((Na % bn) || (Nb % bn) || (r.pair_lds && (size_t)(TF_BM + bn) * K * 2 > TF_LDS_MAX)) continue;
    const long blocks = (long)(Na / bn) * ((Ma + rpba - 1) / rpba) + (long)(Nb / bn) * ((Mb + 31) / 32);
    if (r.pair_lds) best = bn;
    if (blocks <= 256) { best = bn; break; }
  }
  return best;
}

// ---- the instantiated kernels that a route names (each for BF16 and F16) ----------------------------------------------------------------
// The executors' ladders (tfam_kernels.h) compile the whole BN x KD product of each (PRO, EPI) pair they serve; listed here are the
// instantiations that some supported shape reaches.  The gaps: at K = 768 the 16- and the 32-column tile of a row-wise launch fill a
// resident round at the same grid, so the picker goes from 16 to 48 / 64; 48 does not divide the 1024 K|V columns of d_model 512; one
// query tile (T <= 16: two clips per block) with more than 16 keys per clip has a V image of more than 48 rows, which only the 16-column
// kernels take, and with four key tiles it fits at d_model 512 only.
enum TfamFamily {
  TFAM_NONE,         // no launch (a step the configuration does not have)
  TFAM_SINGLE,       // tf_gemm_kernel<T, BN, PRO, EPI, KD, DH, QT, NKT, TF_NW, TR>: whole K in LDS
  TFAM_PAIR,         // tf_gemm_pair_kernel<T, BN, PRO, EPI, KD, TF_NW, TR>: two problems in one grid
  TFAM_RING,         // tf_gemm_ring_kernel<T, BN, KC, NST, TR>
  TFAM_POOL,         // tf_pool_kernel<T, KD>
  TFAM_HEAD_BWD1,    // tr_head_bwd1_kernel<T, MAXB>
  TFAM_HEAD_BWD2,    // tr_head_bwd2_kernel<T, MAXB>
  TFAM_HEAD_BWD3,    // tr_head_bwd3_kernel<KD>
  TFAM_WGRAD,        // tr_wgrad_group_kernel<T>
};
// Template arguments a kernel does not take are 0; launches without attention pass DH 64, QT 1, NKT 1.  bound: __launch_bounds__.
struct TfamInst { int family, bn, pro, epi, kd, dh, qt, nkt, tr, kc, maxb, bound; };
#define TFAM_S(bn, pro, epi, kd, tr) {TFAM_SINGLE, bn, pro, epi, kd, 64, 1, 1, tr, 0, 0, 64 * TF_NW}
#define TFAM_S2(bn, pro, epi, tr) TFAM_S(bn, pro, epi, 512, tr), TFAM_S(bn, pro, epi, 768, tr)
#define TFAM_A(bn, kd, dh, qt, nkt, tr) {TFAM_SINGLE, bn, PRO_ATTN, EPI_RESID32, kd, dh, qt, nkt, tr, 0, 0, 64 * TF_NW}
#define TFAM_A4(bn, qt, nkt, tr) TFAM_A(bn, 512, 64, qt, nkt, tr), TFAM_A(bn, 768, 64, qt, nkt, tr), TFAM_A(bn, 768, 96, qt, nkt, tr)
#define TFAM_P(bn, pro, kd, tr) {TFAM_PAIR, bn, pro, EPI_ACT16, kd, 0, 0, 0, tr, 0, 0, 64 * TF_NW}
#define TFAM_P2(bn, pro, tr) TFAM_P(bn, pro, 512, tr), TFAM_P(bn, pro, 768, tr)
constexpr TfamInst kTfamInsts[] = {
    // eval chain
    TFAM_S2(16, PRO_F32, EPI_ACT16, 0), TFAM_S(32, PRO_F32, EPI_ACT16, 512, 0), TFAM_S2(48, PRO_F32, EPI_ACT16, 0), TFAM_S2(64, PRO_F32, EPI_ACT16, 0),
    TFAM_S2(16, PRO_LN, EPI_ACT16, 0), TFAM_S(32, PRO_LN, EPI_ACT16, 512, 0), TFAM_S2(48, PRO_LN, EPI_ACT16, 0), TFAM_S2(64, PRO_LN, EPI_ACT16, 0),
    TFAM_S2(16, PRO_16, EPI_ACT16, 0), TFAM_S(16, PRO_16, EPI_BIAS32, 256, 0), TFAM_S(16, PRO_16, EPI_BIAS32, 384, 0),
    TFAM_A4(16, 1, 1, 0), TFAM_A4(16, 1, 2, 0), TFAM_A4(16, 2, 1, 0), TFAM_A4(16, 2, 2, 0), TFAM_A(16, 512, 64, 1, 4, 0), TFAM_A4(16, 2, 4, 0),
    TFAM_A4(32, 1, 1, 0), TFAM_A4(32, 2, 1, 0), TFAM_A4(32, 2, 2, 0),
    TFAM_P2(16, PRO_F32, 0), TFAM_P2(32, PRO_F32, 0), TFAM_P(48, PRO_F32, 768, 0), TFAM_P2(64, PRO_F32, 0),
    TFAM_P2(16, PRO_LN, 0), TFAM_P2(32, PRO_LN, 0), TFAM_P(48, PRO_LN, 768, 0), TFAM_P2(64, PRO_LN, 0),
    {TFAM_RING, TF_RING_BN, 0, 0, 0, 0, 0, 0, 0, TF_RING_KC, 0, TF_NTH},
    // training chains
    TFAM_S2(16, PRO_F32, EPI_ACT16, 1), TFAM_S(32, PRO_F32, EPI_ACT16, 512, 1), TFAM_S2(64, PRO_F32, EPI_ACT16, 1),
    TFAM_S2(16, PRO_LN, EPI_ACT16, 1), TFAM_S2(32, PRO_LN, EPI_ACT16, 1), TFAM_S2(64, PRO_LN, EPI_ACT16, 1),
    TFAM_S2(16, PRO_LNBWD, EPI_ACT16, 1), TFAM_S2(32, PRO_LNBWD, EPI_ACT16, 1), TFAM_S2(64, PRO_LNBWD, EPI_ACT16, 1),
    TFAM_S2(16, PRO_16, EPI_ACT16, 1), TFAM_S2(16, PRO_16, EPI_RESID32, 1), TFAM_S(64, PRO_16, EPI_RESID32, 768, 1),
    TFAM_S(16, PRO_16, EPI_BIAS32, 256, 1), TFAM_S(16, PRO_16, EPI_BIAS32, 384, 1),
    TFAM_A4(16, 1, 1, 1), TFAM_A4(16, 1, 2, 1), TFAM_A4(16, 2, 1, 1), TFAM_A4(16, 2, 2, 1), TFAM_A(16, 512, 64, 1, 4, 1), TFAM_A4(16, 2, 4, 1),
    TFAM_P2(32, PRO_F32, 1), TFAM_P2(64, PRO_F32, 1), TFAM_P2(32, PRO_LN, 1), TFAM_P2(64, PRO_LN, 1),
    {TFAM_RING, TF_RING_BN, 0, 0, 0, 0, 0, 0, 1, TF_RING_KC, 0, TF_NTH}, {TFAM_RING, TF_RING_BN, 0, 0, 0, 0, 0, 0, 1, TR_RING_KC_ALT, 0, TF_NTH},
    // both chains
    {TFAM_POOL, 0, 0, 0, 512, 0, 0, 0, 0, 0, 0, 256}, {TFAM_POOL, 0, 0, 0, 768, 0, 0, 0, 0, 0, 0, 256},
    {TFAM_HEAD_BWD1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 8, 512}, {TFAM_HEAD_BWD1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 16, 512}, {TFAM_HEAD_BWD1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 32, 512},
    {TFAM_HEAD_BWD2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 8, 512}, {TFAM_HEAD_BWD2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 16, 512}, {TFAM_HEAD_BWD2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 32, 512},
    {TFAM_HEAD_BWD3, 0, 0, 0, 512, 0, 0, 0, 1, 0, 0, 256}, {TFAM_HEAD_BWD3, 0, 0, 0, 768, 0, 0, 0, 1, 0, 0, 256},
    {TFAM_WGRAD, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, TR_WGRAD_NTH},
};
#undef TFAM_S
#undef TFAM_S2
#undef TFAM_A
#undef TFAM_A4
#undef TFAM_P
#undef TFAM_P2
constexpr int kTfamInstCount = sizeof(kTfamInsts) / sizeof(kTfamInsts[0]);

// ---- one launch ---------------------------------------------------------------------------------------------------------------------
struct TfamPlan {
  int rc = 0;                     // a VMC error code; 0: the fields below are the launch (family TFAM_NONE: nothing to launch)
  int family = TFAM_NONE;
  int bn = 0, pro = 0, epi = 0, kd = 0, dh = 0, qt = 0, nkt = 0, tr = 0, kc = 0, maxb = 0;      // the template arguments, as TfamInst
  unsigned grid = 0;
  int block = 0;
  int lds = 0;                    // dynamic LDS bytes
  int n_tiles = 0, n_rb = 0;      // column tiles and row blocks of the GEMM (pair: of problem a) ...
  int n_tiles_b = 0, n_rb_b = 0;  // ... and of a pair's problem b
};
static inline TfamPlan tfam_error(int rc) {
  TfamPlan p;
  p.rc = rc;
  return p;
}
// index of the plan's kernel in kTfamInsts, -1 when there is none (the CPU test's question; the executors switch on the fields)
static inline int tfam_find_inst(const TfamPlan& p) {
  for (int i = 0; i < kTfamInstCount; ++i) {
    const TfamInst& k = kTfamInsts[i];
    if (k.family == p.family && k.bn == p.bn && k.pro == p.pro && k.epi == p.epi && k.kd == p.kd && k.dh == p.dh && k.qt == p.qt &&
        k.nkt == p.nkt && k.tr == p.tr && k.kc == p.kc && k.maxb == p.maxb)
      return i;
  }
  return -1;
}

// Single-shot GEMM out[M, N] = pro(A)[M, K] W[N, K]^T in row blocks of rpb rows: the whole K of both operands in LDS.
static inline TfamPlan tfam_plan_single(int bn, int pro, int epi, int M, int N, int K, int rpb, bool tr) {
  if (K != 768 && K != 512 && !(pro == PRO_16 && (K == 384 || K == 256))) return tfam_error(VMC_E_SHAPE);      // the instantiated K
  if (tr && bn != 16 && N % bn) return tfam_error(VMC_E_SHAPE);      // training kernels: a ragged last tile (140 classes) only at 16 columns
  const size_t lds = tfam_lds_bytes(bn, false, K, 1, 1, 0);
  if (lds > TF_LDS_MAX) return tfam_error(VMC_E_SHAPE);
  if ((TF_NW / 2 - 1) * 2 * (bn / 16) * 1024 > TF_BM * K * 2) return tfam_error(VMC_E_SHAPE);      // K-slice exchange must fit the A image
  TfamPlan p;
  p.family = TFAM_SINGLE;
  p.bn = bn; p.pro = pro; p.epi = epi; p.kd = K; p.dh = 64; p.qt = 1; p.nkt = 1; p.tr = tr;
  p.n_tiles = (N + bn - 1) / bn;
  p.n_rb = (M + rpb - 1) / rpb;
  p.grid = (unsigned)(p.n_tiles * p.n_rb);
  p.block = 64 * TF_NW;
  p.lds = (int)lds;
  return p;
}
// y = resid + attention(q, k, v) Wo^T + b: the attention of a row block's clips is the prologue of the out-projection (N = K = D).
static inline TfamPlan tfam_plan_attn(int bn, int D, const TfamBlocks& b, int Tk, int nkt, bool tr) {
  if (nkt == 4 && bn != 16) return tfam_error(VMC_E_SHAPE);      // four key tiles: only the 16-column kernels (V and W share a region)
  const size_t lds = tfam_lds_bytes(bn, true, D, nkt, b.cpb, Tk);
  if (lds > TF_LDS_MAX) return tfam_error(VMC_E_SHAPE);
  if ((TF_NW / 2 - 1) * 2 * (bn / 16) * 1024 > TF_BM * D * 2) return tfam_error(VMC_E_SHAPE);
  TfamPlan p;
  p.family = TFAM_SINGLE;
  p.bn = bn; p.pro = PRO_ATTN; p.epi = EPI_RESID32; p.kd = D; p.dh = b.dh; p.qt = b.qt; p.nkt = nkt; p.tr = tr;
  p.n_tiles = (D + bn - 1) / bn;
  p.n_rb = b.n_rb_attn;
  p.grid = (unsigned)(p.n_tiles * p.n_rb);
  p.block = 64 * TF_NW;
  p.lds = (int)lds;
  return p;
}
// Two single-shot problems with the same K, prologue and epilogue in one grid: a's blocks first; b in 32-row blocks.
static inline TfamPlan tfam_plan_pair(int bn, int pro, int Ma, int Na, int rpba, int Mb, int Nb, int K, bool tr) {
  if (K != 768 && K != 512) return tfam_error(VMC_E_SHAPE);
  if ((Na % bn) || (Nb % bn)) return tfam_error(VMC_E_SHAPE);
  const size_t lds = tfam_lds_bytes(bn, false, K, 1, 1, 0);
  if (lds > TF_LDS_MAX) return tfam_error(VMC_E_SHAPE);
  TfamPlan p;
  p.family = TFAM_PAIR;
  p.bn = bn; p.pro = pro; p.epi = EPI_ACT16; p.kd = K; p.tr = tr;
  p.n_tiles = Na / bn; p.n_rb = (Ma + rpba - 1) / rpba;
  p.n_tiles_b = Nb / bn; p.n_rb_b = (Mb + 31) / 32;
  p.grid = (unsigned)(p.n_tiles * p.n_rb + p.n_tiles_b * p.n_rb_b);
  p.block = 64 * TF_NW;
  p.lds = (int)lds;
  return p;
}
// out = resid + A[M, K] W[N, K]^T + b for a K too long for LDS: a ring of K chunks.  The eval chain has KC = 512 only.
static inline TfamPlan tfam_plan_ring(int M, int N, int K, int rpb, bool tr) {
  const int kc = K % TF_RING_KC == 0 ? TF_RING_KC : (tr && K % TR_RING_KC_ALT == 0) ? TR_RING_KC_ALT : 0;
  if (!kc) return tfam_error(VMC_E_SHAPE);
  const size_t lds = (size_t)TF_RING_NST * (TF_BM + TF_RING_BN) * kc * 2 + 2 * (TF_RING_BN / 16) * 1024;
  if (lds > TF_LDS_MAX) return tfam_error(VMC_E_SHAPE);
  TfamPlan p;
  p.family = TFAM_RING;
  p.bn = TF_RING_BN; p.kc = kc; p.tr = tr;
  p.n_tiles = (N + TF_RING_BN - 1) / TF_RING_BN;
  p.n_rb = (M + rpb - 1) / rpb;
  p.grid = (unsigned)(p.n_tiles * p.n_rb);
  p.block = TF_NTH;
  p.lds = (int)lds;
  return p;
}
static inline TfamPlan tfam_plan_small(int family, int kd, int maxb, int tr, unsigned grid, int block, size_t lds) {
  TfamPlan p;
  p.family = family; p.kd = kd; p.maxb = maxb; p.tr = tr;
  p.grid = grid; p.block = block; p.lds = (int)lds;
  return p;
}

// ---- the steps of the chains --------------------------------------------------------------------------------------------------------
// A step's launches in order; a launch the configuration does not have (cross attention off, layer 0's dx) has family TFAM_NONE.
// rc: the first non-zero rc of its launches.
template <int N>
struct TfamStep {
  TfamPlan p[N];
  int rc = 0;
  static constexpr int count = N;
};
template <int N>
static inline TfamStep<N> tfam_step_done(TfamStep<N> s) {
  for (int i = 0; i < N && !s.rc; ++i) s.rc = s.p[i].rc;
  return s;
}

// One AttentionLayer forward (tfam_fused.hip / tfam_train.hip head comments): 1 qkv, 2 self attention + out-projection, 3 cross q,
// 4 cross attention + out-projection, 5 ffn.0, 6 ffn.3.  first: layer 0 reads the fp32 tokens (PRO_F32), later layers the previous
// layer's LayerNorm (PRO_LN).  pair: the layer's K|V projection of the motion tokens rides the qkv launch (vmc_tfam_forward and the
// training chain; vmc_tfam_layer_fwd leaves it to vmc_tfam_kv_fwd).
enum { TFAM_F_QKV, TFAM_F_SELF, TFAM_F_Q, TFAM_F_CROSS, TFAM_F_FFN0, TFAM_F_FFN3, TFAM_F_COUNT };
static inline TfamStep<TFAM_F_COUNT> tfam_route_layer_fwd(const TfDims& d, const TfamBlocks& b, bool first, bool pair, bool train,
                                                          const TfamOverrides& ov) {
  const TfamTileRule& r = train ? kTfamTrainTiles : kTfamEvalTiles;
  const int D = d.D, M = b.M, rpb = b.rpb, pro1 = first ? PRO_F32 : PRO_LN;
  TfamStep<TFAM_F_COUNT> s;
  if (pair && d.has_cross)
    s.p[TFAM_F_QKV] = tfam_plan_pair(tfam_pick_bn_pair(r, M, 3 * D, rpb, b.Mk, 2 * D, D), pro1, M, 3 * D, rpb, b.Mk, 2 * D, D, train);
  else
    s.p[TFAM_F_QKV] = tfam_plan_single(tfam_pick_bn(r, ov, M, 3 * D, rpb, D, false, !first), pro1, EPI_ACT16, M, 3 * D, D, rpb, train);
  s.p[TFAM_F_SELF] = tfam_plan_attn(tfam_pick_bn(r, ov, M, D, rpb, D, true, false, b.vrows), D, b, d.T, b.nkt, train);
  if (d.has_cross) {
    s.p[TFAM_F_Q] = tfam_plan_single(tfam_pick_bn(r, ov, M, D, rpb, D, false, true), PRO_LN, EPI_ACT16, M, D, D, rpb, train);
    s.p[TFAM_F_CROSS] = tfam_plan_attn(tfam_pick_bn(r, ov, M, D, rpb, D, true, false, b.vrows_x), D, b, d.Tk, b.nkt_x, train);
  }
  s.p[TFAM_F_FFN0] = tfam_plan_single(tfam_pick_bn(r, ov, M, d.ff, rpb, D, false, true), PRO_LN, EPI_ACT16, M, d.ff, D, rpb, train);
  s.p[TFAM_F_FFN3] = tfam_plan_ring(M, D, d.ff, rpb, train);
  return tfam_step_done(s);
}
// vmc_tfam_kv_fwd: one layer's stand-alone K|V projection of the motion tokens (eval chain)
static inline TfamPlan tfam_route_kv(const TfDims& d, const TfamBlocks& b, const TfamOverrides& ov) {
  return tfam_plan_single(tfam_pick_bn(kTfamEvalTiles, ov, b.Mk, 2 * d.D, 32, d.D, false, false), PRO_F32, EPI_ACT16, b.Mk, 2 * d.D, d.D, 32, false);
}

// Head forward: mean-pool + the two LayerNorms, classifier.1 (GELU), classifier.4 (fp32 logits; a ragged last tile of classes).
// The eval chain's two GEMMs take the 16-column tile; the training chain picks.
enum { TFAM_H_POOL, TFAM_H_CLS1, TFAM_H_CLS4, TFAM_H_COUNT };
static inline TfamStep<TFAM_H_COUNT> tfam_route_head_fwd(const TfDims& d, bool train, const TfamOverrides& ov) {
  const int D = d.D;
  TfamStep<TFAM_H_COUNT> s;
  s.p[TFAM_H_POOL] = tfam_plan_small(TFAM_POOL, D, 0, 0, (unsigned)d.B, 256, 0);
  const int bn1 = train ? tfam_pick_bn(kTfamTrainTiles, ov, d.B, D / 2, 32, D, false, false) : 16;
  const int bn4 = train ? tfam_pick_bn(kTfamTrainTiles, ov, d.B, d.C, 32, D / 2, false, false) : 16;
  s.p[TFAM_H_CLS1] = tfam_plan_single(bn1, PRO_16, EPI_ACT16, d.B, D / 2, D, 32, train);
  s.p[TFAM_H_CLS4] = tfam_plan_single(bn4, PRO_16, EPI_BIAS32, d.B, d.C, D / 2, 32, train);
  return tfam_step_done(s);
}

// Head backward (tfam_train.hip): H1 (classifier.4, dlogits rows in LDS), H2 (classifier.1), H3 (LayerNorm_cls + mean-pool).
static inline TfamStep<3> tfam_route_head_bwd(const TfDims& d) {
  const int D = d.D, Dh = D / 2, C = d.C;
  TfamStep<3> s;
  if ((size_t)TR_MAX_B * C * sizeof(float) > (size_t)TR_HEAD_LDS_MAX || d.B > TR_MAX_B) {      // tfam_check 8, 9
    s.p[0] = tfam_error(VMC_E_SHAPE);
    return tfam_step_done(s);
  }
  const int mb = d.B <= 8 ? 8 : d.B <= 16 ? 16 : 32;
  s.p[0] = tfam_plan_small(TFAM_HEAD_BWD1, 0, mb, 1, (unsigned)(Dh / 64 + (C * Dh + C + 511) / 512), 512, (512 + (size_t)mb * C) * sizeof(float));
  s.p[1] = tfam_plan_small(TFAM_HEAD_BWD2, 0, mb, 1, (unsigned)(D / 64 + (Dh * D + Dh + 511) / 512), 512, (512 + (size_t)mb * Dh) * sizeof(float));
  s.p[2] = tfam_plan_small(TFAM_HEAD_BWD3, D, 0, 1, (unsigned)(d.B + 1), 256, 0);
  return tfam_step_done(s);
}

// One layer's dgrad chain (tfam_train.hip head comment): L1 dh, L2 dx2 (K = ff ring), L3 dOc, [L4 attention backward], L5 dx1,
// L6 dOs, [L7 attention backward], L8 dx of the layer below (K = 3D ring; not for layer 0).  L4 / L7 are vmc_attention_bwd calls
// (attn_route.h).  All launches are row-wise: uniform blocks of rpb rows.
enum { TFAM_B_DH, TFAM_B_DX2, TFAM_B_DOC, TFAM_B_DX1, TFAM_B_DOS, TFAM_B_DX0, TFAM_B_COUNT };
static inline TfamStep<TFAM_B_COUNT> tfam_route_layer_bwd(const TfDims& d, const TfamBlocks& b, bool first, const TfamOverrides& ov) {
  const TfamTileRule& r = kTfamTrainTiles;
  const int D = d.D, M = b.M, rpb = b.rpb;
  TfamStep<TFAM_B_COUNT> s;
  s.p[TFAM_B_DH] = tfam_plan_single(tfam_pick_bn(r, ov, M, d.ff, rpb, D, false, true), PRO_LNBWD, EPI_ACT16, M, d.ff, D, rpb, true);
  s.p[TFAM_B_DX2] = tfam_plan_ring(M, D, d.ff, rpb, true);
  const int bn_d = tfam_pick_bn(r, ov, M, D, rpb, D, false, true);
  if (d.has_cross) {
    s.p[TFAM_B_DOC] = tfam_plan_single(bn_d, PRO_LNBWD, EPI_ACT16, M, D, D, rpb, true);
    s.p[TFAM_B_DX1] = tfam_plan_single(tfam_pick_bn(r, ov, M, D, rpb, D, false, false), PRO_16, EPI_RESID32, M, D, D, rpb, true);
  }
  s.p[TFAM_B_DOS] = tfam_plan_single(bn_d, PRO_LNBWD, EPI_ACT16, M, D, D, rpb, true);
  if (!first) s.p[TFAM_B_DX0] = tfam_plan_ring(M, D, 3 * D, rpb, true);
  return tfam_step_done(s);
}

// Grouped weight gradients: dW = dY^T X in 256 x 128 tiles, problems in the order qkv, self out, [cross q, cross k|v, cross out,]
// ffn.0, ffn.3, then the layer's LayerNorm problems (64 columns per workgroup) ffn, [cross,] self.  The LayerNorm blocks come FIRST in
// the grid.  vmc_tfam_train_bwd defers the problems of up to TR_WGRAD_FLUSH layers into one launch; vmc_tfam_layer_bwd launches its own.
static inline int tfam_tn_tiles_k(int K) { return (K + 127) / 128; }
static inline int tfam_tn_tiles(int N, int K) { return ((N + 255) / 256) * tfam_tn_tiles_k(K); }
struct TfamWgradLayer {
  int nprob, nln;
  int tiles[TR_WGRAD_PROBS];
};
static inline TfamWgradLayer tfam_wgrad_layer(const TfDims& d) {
  const int D = d.D;
  TfamWgradLayer w = {};
  w.tiles[w.nprob++] = tfam_tn_tiles(3 * D, D);
  w.tiles[w.nprob++] = tfam_tn_tiles(D, D);
  if (d.has_cross) {
    w.tiles[w.nprob++] = tfam_tn_tiles(D, D);
    w.tiles[w.nprob++] = tfam_tn_tiles(2 * D, D);
    w.tiles[w.nprob++] = tfam_tn_tiles(D, D);
  }
  w.tiles[w.nprob++] = tfam_tn_tiles(d.ff, D);
  w.tiles[w.nprob++] = tfam_tn_tiles(D, d.ff);
  w.nln = d.has_cross ? 3 : 2;
  return w;
}
// the launch for `layers` deferred layers with every gradient requested (a problem without a gradient pointer is left out at run time)
static inline TfamPlan tfam_route_wgrad(const TfDims& d, int layers) {
  const TfamWgradLayer w = tfam_wgrad_layer(d);
  if (layers <= 0 || layers * w.nprob > TR_MAX_PROB || layers * w.nln > TR_MAX_LN) return tfam_error(VMC_E_SHAPE);
  int tiles = 0;
  for (int i = 0; i < w.nprob; ++i) tiles += w.tiles[i];
  return tfam_plan_small(TFAM_WGRAD, 0, 0, 1, (unsigned)(layers * (tiles + w.nln * (d.D / 64))), TR_WGRAD_NTH, TR_WGRAD_LDS);
}
// layers whose problems go into the launch issued after layer l's dgrad chain (l counts down from L - 1), 0: none yet
static inline int tfam_wgrad_flush(int L, int l) {
  const int pending = (L - 1 - l) % TR_WGRAD_FLUSH + 1;
  return (pending == TR_WGRAD_FLUSH || l == 0) ? pending : 0;
}

// ---- the supported set --------------------------------------------------------------------------------------------------------------
// Every shape condition of the chains, in this order; after 0 no launch of that chain returns VMC_E_SHAPE.
//   1  B, T, L, C > 0 and T <= TF_MAX_T                     5  dim_feedforward > 0, a multiple of 512
//   2  d_model 512 or 768                                   6  cross attention: 0 < Tk <= TF_MAX_T
//   3  nhead > 0 divides d_model                            7  (clips per row block) * nhead a multiple of 4
//   4  head_dim 64 or 96
//   8  train: B T <= 256 and (cross attention) B Tk <= 256; C a multiple of 4; B <= 32
//   9  train: the head backward's dlogits rows fit its LDS (C <= 480)
//  10  the self attention's and 11 the cross attention's Q | W | V images fit TF_LDS_MAX.  Two clips' keys per row block (T <= 16)
//      are what can exceed it: Tk >= 27 at d_model 768, Tk = 64 at d_model 512.
// 1-7 give every other launch an instantiated K (d_model, d_model / 2; rings over multiples of 512 or 384), a tile that fits LDS
// and the K-slice exchange area, and a weight-gradient group inside its table: none of the routes above returns an error then, which
// tests/host/test_tfam_route.cpp sweeps.
static inline int tfam_check(const TfDims& d, bool train) {
  if (d.B <= 0 || d.T <= 0 || d.T > TF_MAX_T || d.L <= 0 || d.C <= 0) return VMC_E_SHAPE;
  if (d.D != 512 && d.D != 768) return VMC_E_SHAPE;
  if (d.H <= 0 || d.D % d.H) return VMC_E_SHAPE;
  const int dh = d.D / d.H;
  if (dh != 64 && dh != 96) return VMC_E_SHAPE;
  if (d.ff % 512 || d.ff <= 0) return VMC_E_SHAPE;
  if (d.has_cross && (d.Tk <= 0 || d.Tk > TF_MAX_T)) return VMC_E_SHAPE;
  const TfamBlocks b = tfam_blocks(d);
  if ((b.cpb * d.H) % 4) return VMC_E_SHAPE;
  if (train) {
    if (b.M > TR_MAX_ROWS || b.Mk > TR_MAX_ROWS) return VMC_E_SHAPE;
    if (d.C % 4 || d.B > TR_MAX_B) return VMC_E_SHAPE;
    if ((size_t)TR_MAX_B * d.C * sizeof(float) > (size_t)TR_HEAD_LDS_MAX) return VMC_E_SHAPE;
  }
  const TfamTileRule& r = train ? kTfamTrainTiles : kTfamEvalTiles;
  const TfamOverrides none;      // the switches do not reach the attention launches
  if (int rc = tfam_plan_attn(tfam_pick_bn(r, none, b.M, d.D, b.rpb, d.D, true, false, b.vrows), d.D, b, d.T, b.nkt, train).rc) return rc;
  if (d.has_cross)
    if (int rc = tfam_plan_attn(tfam_pick_bn(r, none, b.M, d.D, b.rpb, d.D, true, false, b.vrows_x), d.D, b, d.Tk, b.nkt_x, train).rc) return rc;
  return 0;
}

// ---- workspaces (pure functions of the dims; laid out from a null base the pointers are the offsets) ---------------------------------
// eval chain
// workspace: [y f32 M*D][xa f32 M*D][xb f32 M*D][qkv16 M*3D][q16 M*D][h16 M*ff][kv16 Mk*L*2D][pool16 B*D][g16 B*D/2]
//            [q frag][self-k frag][cross-k frag x L]   (fragment-major, tf_frag_off; the row-major q / k columns stay unused)
struct TfWs {
  float *y, *xa, *xb;
  uint16_t *qkv, *q, *h, *kv, *pool, *g;
  uint16_t *qf, *kf, *kxf;      // fragment-major q, self k, and (per layer) cross k
  size_t kxf_stride;            // elements between two layers' cross-k buffers
  size_t bytes;
};
static inline TfWs tf_ws(void* base, const TfDims& d) {
  const size_t M = (size_t)d.B * d.T, Mk = (size_t)d.B * (d.has_cross ? d.Tk : 0);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  char* p = (char*)base;
  TfWs w;
  size_t o = 0;
  w.y = (float*)(p + o); o += al(M * d.D * 4);
  w.xa = (float*)(p + o); o += al(M * d.D * 4);
  w.xb = (float*)(p + o); o += al(M * d.D * 4);
  w.qkv = (uint16_t*)(p + o); o += al(M * 3 * d.D * 2);
  w.q = (uint16_t*)(p + o); o += al(M * d.D * 2);
  w.h = (uint16_t*)(p + o); o += al(M * d.ff * 2);
  w.kv = (uint16_t*)(p + o); o += al(Mk * d.L * 2 * d.D * 2);
  w.pool = (uint16_t*)(p + o); o += al((size_t)d.B * d.D * 2);
  w.g = (uint16_t*)(p + o); o += al((size_t)d.B * (d.D / 2) * 2);
  const int H = d.H > 0 ? d.H : 8, dh = d.D / H;
  const size_t fe = tf_frag_elems(d.B, H, dh, tf_ntt(d.T > d.Tk ? d.T : d.Tk));
  w.qf = (uint16_t*)(p + o); o += al(fe * 2);
  w.kf = (uint16_t*)(p + o); o += al(fe * 2);
  w.kxf = (uint16_t*)(p + o); w.kxf_stride = al(fe * 2) / 2; o += (d.has_cross ? d.L : 0) * al(fe * 2);
  w.bytes = o;
  return w;
}

static inline size_t tfam_workspace_bytes(const TfDims& d) { return tf_ws(nullptr, d).bytes; }

// training chains
struct TrLayerWs {
  // saved by the forward
  float* xin32;             // layer > 0: LN_ffn[l-1](y3[l-1]) (the residual operand; layer 0 uses the caller's tokens)
  uint16_t* x0_16;          // 16-bit rows fed to the qkv GEMM
  uint16_t* qkv16;          // [M, 3D]
  uint16_t* o_self;         // [M, D]
  float* lse_self;          // [B, H, T]
  float* y1;                // pre-norm sums (fp32)
  uint8_t* keep1;
  float* x1_32;
  uint16_t* x1_16;
  uint16_t* q16;            // [M, D]
  uint16_t* kv16;           // [Mk, 2D]
  uint16_t* o_cross;
  float* lse_cross;
  float* y2;
  uint8_t* keep2;
  float* x2_32;
  uint16_t* x2_16;
  uint16_t* h16;            // [M, ff] after ReLU and dropout
  float* y3;
  uint8_t* keep3;
  // backward
  float *dx3, *dy3, *dx2, *dy2, *dx1, *dy1;
  uint16_t *d3_16, *dh16, *d2_16, *doc16, *dq16, *dkv16, *d1_16, *dos16, *dqkv16;
  float *st3, *st2, *st1;   // [M, 2] mean, rstd
  float* attn_ws;
};
struct TrWs {
  uint16_t* motion16;       // [Mk, D]
  uint16_t *qf, *kf, *kxf;  // fragment-major q / k operands of the fused attention prologues (forward-only)
  float* pooled32;          // [B, D]
  uint16_t* pool16;         // [B, D]   LN_cls(pooled) 16-bit
  uint16_t* a16;            // [B, D/2] classifier.1 pre-activation
  uint16_t* g16;            // [B, D/2] drop(gelu(a))
  float* da;                // [B, D/2]
  float* dpl;               // [B, D]   gradient wrt LN_cls(pooled)
  char* layers;
  size_t layer_bytes;
  size_t bytes;
};

static inline size_t tr_al(size_t x) { return (x + 255) & ~(size_t)255; }

static inline TrLayerWs tr_layer_ws(char* base, const TfDims& d, size_t* bytes_out = nullptr) {
  const size_t M = (size_t)d.B * d.T, Mk = (size_t)d.B * (d.has_cross ? d.Tk : 0), D = d.D, ff = d.ff;
  TrLayerWs w;
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base + o; o += tr_al(n); return p; };
  w.xin32 = (float*)take(M * D * 4);
  w.x0_16 = (uint16_t*)take(M * D * 2);
  w.qkv16 = (uint16_t*)take(M * 3 * D * 2);
  w.o_self = (uint16_t*)take(M * D * 2);
  w.lse_self = (float*)take((size_t)d.B * d.H * d.T * 4);
  w.y1 = (float*)take(M * D * 4);
  w.keep1 = (uint8_t*)take(M * D);
  w.x1_32 = (float*)take(M * D * 4);
  w.x1_16 = (uint16_t*)take(M * D * 2);
  w.q16 = (uint16_t*)take(M * D * 2);
  w.kv16 = (uint16_t*)take(Mk * 2 * D * 2);
  w.o_cross = (uint16_t*)take(M * D * 2);
  w.lse_cross = (float*)take((size_t)d.B * d.H * d.T * 4);
  w.y2 = (float*)take(M * D * 4);
  w.keep2 = (uint8_t*)take(M * D);
  w.x2_32 = (float*)take(M * D * 4);
  w.x2_16 = (uint16_t*)take(M * D * 2);
  w.h16 = (uint16_t*)take(M * ff * 2);
  w.y3 = (float*)take(M * D * 4);
  w.keep3 = (uint8_t*)take(M * D);
  w.dx3 = (float*)take(M * D * 4);
  w.dy3 = (float*)take(M * D * 4);
  w.dx2 = (float*)take(M * D * 4);
  w.dy2 = (float*)take(M * D * 4);
  w.dx1 = (float*)take(M * D * 4);
  w.dy1 = (float*)take(M * D * 4);
  w.d3_16 = (uint16_t*)take(M * D * 2);
  w.dh16 = (uint16_t*)take(M * ff * 2);
  w.d2_16 = (uint16_t*)take(M * D * 2);
  w.doc16 = (uint16_t*)take(M * D * 2);
  w.dq16 = (uint16_t*)take(M * D * 2);
  w.dkv16 = (uint16_t*)take(Mk * 2 * D * 2);
  w.d1_16 = (uint16_t*)take(M * D * 2);
  w.dos16 = (uint16_t*)take(M * D * 2);
  w.dqkv16 = (uint16_t*)take(M * 3 * D * 2);
  w.st3 = (float*)take(M * 2 * 4);
  w.st2 = (float*)take(M * 2 * 4);
  w.st1 = (float*)take(M * 2 * 4);
  w.attn_ws = (float*)take((size_t)d.B * d.H * d.T * 4);
  if (bytes_out) *bytes_out = o;
  return w;
}

static inline TrWs tr_ws(void* base, const TfDims& d) {
  const size_t Mk = (size_t)d.B * (d.has_cross ? d.Tk : 0), D = d.D;
  char* p = (char*)base;
  TrWs w;
  size_t o = 0;
  auto take = [&](size_t n) { char* q = p + o; o += tr_al(n); return q; };
  w.motion16 = (uint16_t*)take(Mk * D * 2);
  const size_t fe = tf_frag_elems(d.B, d.H, d.D / d.H, tf_ntt(d.T > d.Tk ? d.T : d.Tk));
  w.qf = (uint16_t*)take(fe * 2);
  w.kf = (uint16_t*)take(fe * 2);
  w.kxf = (uint16_t*)take(fe * 2);
  w.pooled32 = (float*)take((size_t)d.B * D * 4);
  w.pool16 = (uint16_t*)take((size_t)d.B * D * 2);
  w.a16 = (uint16_t*)take((size_t)d.B * (D / 2) * 2);
  w.g16 = (uint16_t*)take((size_t)d.B * (D / 2) * 2);
  w.da = (float*)take((size_t)d.B * (D / 2) * 4);
  w.dpl = (float*)take((size_t)d.B * D * 4);
  tr_layer_ws(nullptr, d, &w.layer_bytes);
  w.layers = p + o;
  o += (size_t)d.L * w.layer_bytes;
  w.bytes = o;
  return w;
}
static inline TrLayerWs tr_lw(const TrWs& w, const TfDims& d, int layer) { return tr_layer_ws(w.layers + (size_t)layer * w.layer_bytes, d); }

static inline size_t tfam_train_workspace_bytes(const TfDims& d) { return tr_ws(nullptr, d).bytes; }
// offset of the gradient wrt the pooled rows (dx3 of the last layer): where a caller adds gradients of other heads
static inline long long tfam_train_pool_grad_offset(const TfDims& d) {
  const TrWs ws = tr_ws(nullptr, d);
  return (long long)(uintptr_t)tr_lw(ws, d, d.L - 1).dx3;
}

// ---- feature-concatenation mode: projection_layer in front of layer 0 (training chains) --------------------------------------------
// AMO_CLIP with use_cross_attention = false, concat_dim = -1 (TFAM/models/AMO_CLIP.py:153-157): x = Linear(2 D, D)(cat(rgb, motion)).
// The chain's input is the materialised xcat [M, 2 D] fp32.  What it adds to the training chains of a model without cross attention:
//   F0     x32 = 16bit(xcat) Wp^T + bp   one single-shot launch in front of layer 0 (K = 2 D; side output xcat16), 32-row blocks
//   L8(0)  dx0 = dy1 + dqkv Wqkv         layer 0 runs the K = 3 D ring that the other layers run, with a 16-bit side output d0_16
//   one more problem (d0_16^T xcat16 -> projection weight and bias gradient) in the grouped launch that holds layer 0's problems
// Their kernels live in a table of their own: kTfamInsts lists what the shapes WITHOUT a projection reach.
constexpr TfamInst kTfamProjInsts[] = {
    {TFAM_SINGLE, 16, PRO_F32, EPI_BIAS32, 1024, 64, 1, 1, 1, 0, 0, 64 * TF_NW},
    {TFAM_SINGLE, 16, PRO_F32, EPI_BIAS32, 1536, 64, 1, 1, 1, 0, 0, 64 * TF_NW},
};
constexpr int kTfamProjInstCount = sizeof(kTfamProjInsts) / sizeof(kTfamProjInsts[0]);
static inline int tfam_find_proj_inst(const TfamPlan& p) {
  for (int i = 0; i < kTfamProjInstCount; ++i) {
    const TfamInst& k = kTfamProjInsts[i];
    if (k.family == p.family && k.bn == p.bn && k.pro == p.pro && k.epi == p.epi && k.kd == p.kd && k.dh == p.dh && k.qt == p.qt &&
        k.nkt == p.nkt && k.tr == p.tr && k.kc == p.kc && k.maxb == p.maxb)
      return i;
  }
  return -1;
}

// F0.  The 16-column tile is the only one whose A and W images of K = 1536 fit TF_LDS_MAX ((32 + 16) x 1536 x 2 B = 147 456 B).
static inline TfamPlan tfam_route_proj_fwd(const TfDims& d) {
  const int K = 2 * d.D, bn = 16, M = d.B * d.T;
  if (K != 1024 && K != 1536) return tfam_error(VMC_E_SHAPE);      // the instantiated K
  const size_t lds = tfam_lds_bytes(bn, false, K, 1, 1, 0);
  if (lds > TF_LDS_MAX) return tfam_error(VMC_E_SHAPE);
  if ((TF_NW / 2 - 1) * 2 * (bn / 16) * 1024 > TF_BM * K * 2) return tfam_error(VMC_E_SHAPE);
  TfamPlan p;
  p.family = TFAM_SINGLE;
  p.bn = bn; p.pro = PRO_F32; p.epi = EPI_BIAS32; p.kd = K; p.dh = 64; p.qt = 1; p.nkt = 1; p.tr = 1;
  p.n_tiles = d.D / bn;
  p.n_rb = (M + TF_BM - 1) / TF_BM;
  p.grid = (unsigned)(p.n_tiles * p.n_rb);
  p.block = 64 * TF_NW;
  p.lds = (int)lds;
  return p;
}
// L8 of layer 0
static inline TfamPlan tfam_route_proj_bwd(const TfDims& d, const TfamBlocks& b) { return tfam_plan_ring(b.M, d.D, 3 * d.D, b.rpb, true); }
// the grouped launch that holds layer 0's problems (`layers` deferred layers) with the projection's problem behind them
static inline TfamPlan tfam_route_proj_wgrad(const TfDims& d, int layers) {
  TfamPlan p = tfam_route_wgrad(d, layers);
  if (p.rc) return p;
  if (layers * tfam_wgrad_layer(d).nprob + 1 > TR_MAX_PROB) return tfam_error(VMC_E_SHAPE);
  p.grid += (unsigned)tfam_tn_tiles(d.D, 2 * d.D);
  return p;
}
// The supported set: tfam_check(train), and 12 no cross attention, 13 an instantiated K = 2 d_model whose tile fits TF_LDS_MAX,
// 14 L nprob + 1 <= TR_MAX_PROB: every layer's problems and the projection's fit one table (L <= 7 at four problems per layer).
static inline int tfam_check_proj(const TfDims& d) {
  if (int rc = tfam_check(d, true)) return rc;
  if (d.has_cross) return VMC_E_SHAPE;
  if (int rc = tfam_route_proj_fwd(d).rc) return rc;
  if (d.L * tfam_wgrad_layer(d).nprob + 1 > TR_MAX_PROB) return VMC_E_SHAPE;
  return 0;
}

// Workspace extension, laid out BEHIND the training workspace (every offset of tr_ws stays what it is without a projection).
struct TrProjWs {
  float* x32;               // [M, D]   projection output: layer 0's tokens (the residual operand of its F2)
  uint16_t* xcat16;         // [M, 2D]  16-bit cast of the concatenated features: the X operand of the projection's weight gradient
  float* dx0;               // [M, D]   gradient wrt x32
  uint16_t* d0_16;          // [M, D]   its 16-bit copy: the dY operand
  size_t bytes;             // of the whole workspace, tr_ws included
};
static inline TrProjWs tr_proj_ws(void* base, const TfDims& d) {
  const size_t M = (size_t)d.B * d.T, D = d.D;
  char* p = (char*)base;
  TrProjWs w;
  size_t o = tr_ws(nullptr, d).bytes;
  auto take = [&](size_t n) { char* q = p + o; o += tr_al(n); return q; };
  w.x32 = (float*)take(M * D * 4);
  w.xcat16 = (uint16_t*)take(M * 2 * D * 2);
  w.dx0 = (float*)take(M * D * 4);
  w.d0_16 = (uint16_t*)take(M * D * 2);
  w.bytes = o;
  return w;
}
static inline size_t tfam_train_proj_workspace_bytes(const TfDims& d) { return tr_proj_ws(nullptr, d).bytes; }
// offset of dx0 (rows behind the pool length are exactly zero there)
static inline long long tfam_train_proj_dx0_offset(const TfDims& d) { return (long long)(uintptr_t)tr_proj_ws(nullptr, d).dx0; }

// ---- gradients wrt the input tokens (training chains; opt-in: AMO_CLIP.fused_input_grads) -----------------------------------------
// What the backward adds when the caller's token tensors require a gradient.  Nothing above changes: the launches below follow the
// existing ones and write into a workspace extension behind tr_ws (without a projection) or behind tr_proj_ws (with one).
//   dX       [M, D]   fp32  L8 of layer 0, dX = dy1 + dqkv Wqkv: the K = 3 D ring every other layer runs.  Rows at and behind the pool
//                           length are exact zeros (masked as keys, not pooled: no gradient reaches them).
//   dMotion  [Mk, D]  fp32  cross attention: sum over the layers of dkv16_l Wkv_l, K = 2 D ring over a column window of wt_cross_in
//                           (leading dimension 3 D), one launch behind each layer's cross-attention backward.  Layer L - 1 writes, the
//                           layers below add through the launch's residual operand: fp32, one fixed order, bit for bit repeatable.
//   dXcat    [M, 2 D] fp32  projection mode: d0_16 Wp, one single-shot launch behind layer 0's L8 (N = 2 D, K = D, no bias, no residual).
// The single-shot kernel is compiled already (tf_run_single<PRO_16, EPI_BIAS32> builds the whole BN x KD product for the classifier), but
// no shape of kTfamInsts reaches it at K = d_model; it is listed here.
constexpr TfamInst kTfamInputInsts[] = {
    {TFAM_SINGLE, 16, PRO_16, EPI_BIAS32, 512, 64, 1, 1, 1, 0, 0, 64 * TF_NW},
    {TFAM_SINGLE, 16, PRO_16, EPI_BIAS32, 768, 64, 1, 1, 1, 0, 0, 64 * TF_NW},
    {TFAM_RING, TF_RING_BN, 0, 0, 0, 0, 0, 0, 1, TF_RING_KC, 0, TF_NTH},
    {TFAM_RING, TF_RING_BN, 0, 0, 0, 0, 0, 0, 1, TR_RING_KC_ALT, 0, TF_NTH},
};
constexpr int kTfamInputInstCount = sizeof(kTfamInputInsts) / sizeof(kTfamInputInsts[0]);
static inline int tfam_find_input_inst(const TfamPlan& p) {
  for (int i = 0; i < kTfamInputInstCount; ++i) {
    const TfamInst& k = kTfamInputInsts[i];
    if (k.family == p.family && k.bn == p.bn && k.pro == p.pro && k.epi == p.epi && k.kd == p.kd && k.dh == p.dh && k.qt == p.qt &&
        k.nkt == p.nkt && k.tr == p.tr && k.kc == p.kc && k.maxb == p.maxb)
      return i;
  }
  return -1;
}

// dX: L8 of layer 0, the plan of the other layers' L8
static inline TfamPlan tfam_route_input_dx(const TfDims& d, const TfamBlocks& b) { return tfam_plan_ring(b.M, d.D, 3 * d.D, b.rpb, true); }
// dMotion of one layer: the motion rows in uniform 32-row blocks (as the forward's K|V projection); K = 2 D is 1024 or 1536: KC = 512
static inline TfamPlan tfam_route_input_dmotion(const TfDims& d, const TfamBlocks& b) {
  if (!d.has_cross) return TfamPlan();
  return tfam_plan_ring(b.Mk, d.D, 2 * d.D, TF_BM, true);
}
// dXcat.  The 16-column tile: (32 + 16) x 768 x 2 B of LDS lets two workgroups share a CU, and 2 D / 16 x M / 32 <= 768 workgroups
// keep every CU streaming its own rows of Wp^T.
static inline TfamPlan tfam_route_input_dxcat(const TfDims& d) {
  return tfam_plan_single(16, PRO_16, EPI_BIAS32, d.B * d.T, 2 * d.D, d.D, TF_BM, true);
}
// The supported set: that of the chain itself (tfam_check(train), or tfam_check_proj with d.proj), and 15 the launches above plan.
static inline int tfam_check_input(const TfDims& d) {
  if (int rc = d.proj ? tfam_check_proj(d) : tfam_check(d, true)) return rc;
  const TfamBlocks b = tfam_blocks(d);
  if (d.proj) return tfam_route_input_dxcat(d).rc;
  if (int rc = tfam_route_input_dx(d, b).rc) return rc;
  return tfam_route_input_dmotion(d, b).rc;
}

// Workspace extension, laid out BEHIND the training workspace (d.proj: behind the projection's extension).
struct TrInputWs {
  float* dx;                // [M, D]    no projection: gradient wrt the pooled stream's tokens
  float* dmotion;           // [Mk, D]   cross attention: gradient wrt the motion tokens
  float* dxcat;             // [M, 2D]   projection: gradient wrt the concatenated features
  size_t bytes;             // of the whole workspace, tr_ws (and tr_proj_ws) included
};
static inline TrInputWs tr_input_ws(void* base, const TfDims& d) {
  const size_t M = (size_t)d.B * d.T, Mk = (size_t)d.B * (d.has_cross ? d.Tk : 0), D = d.D;
  char* p = (char*)base;
  TrInputWs w = {};
  size_t o = d.proj ? tr_proj_ws(nullptr, d).bytes : tr_ws(nullptr, d).bytes;
  auto take = [&](size_t n) { char* q = p + o; o += tr_al(n); return q; };
  if (d.proj) {
    w.dxcat = (float*)take(M * 2 * D * 4);
  } else {
    w.dx = (float*)take(M * D * 4);
    if (d.has_cross) w.dmotion = (float*)take(Mk * D * 4);
  }
  w.bytes = o;
  return w;
}
static inline size_t tfam_train_input_workspace_bytes(const TfDims& d) { return tr_input_ws(nullptr, d).bytes; }
